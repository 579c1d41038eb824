"""Independent PyTorch-CPU formulation of the PNN graphs (SURVEY.md Appendix B.3's cross-check), built on
torch.nn.functional ops instead of hand-written loops.  Used only to validate the CPU oracle: the two must
agree to <= 1e-3 absolute on seeded random weights and on the reference's two real checkpoints.  `dtype` = np.float64 evaluates
the same graphs in double precision: the high-precision yardstick of the f32 order model (tests/test_order_model.py)."""
import numpy as np
import torch
import torch.nn.functional as F

from context_adaptive_neural_network_based_prediction_amd import weights as wts


def _leaky(x):
    return torch.maximum(0.1 * x, x)          # pnn/tfutils.py:192


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype))


def _conv_same(x, W, b, s):
    """TF conv2d SAME, NHWC weights [k,k,Cin,Cout] -> NCHW torch; asymmetric padding for s = 2 (Appendix B.1)."""
    k = W.shape[0]
    H, Wd = x.shape[2], x.shape[3]
    oh, ow = -(-H // s), -(-Wd // s)
    pth, ptw = max((oh - 1) * s + k - H, 0), max((ow - 1) * s + k - Wd, 0)
    x = F.pad(x, (ptw // 2, ptw - ptw // 2, pth // 2, pth - pth // 2))
    return F.conv2d(x, _t(W.transpose(3, 2, 0, 1), W.dtype), _t(b, b.dtype), stride=s)


def _tconv_same(x, W, b, s):
    """TF conv2d_transpose SAME, weights [k,k,Cout,Cin]: full transposed conv then crop (Appendix B.3)."""
    k = W.shape[0]
    H, Wd = x.shape[2], x.shape[3]
    pb = max((H - 1) * s + k - H * s, 0) // 2
    y = F.conv_transpose2d(x, _t(W.transpose(3, 2, 0, 1), W.dtype), None, stride=s)
    y = y[:, :, pb:pb + H * s, pb:pb + Wd * s]
    return y + _t(b, b.dtype).view(1, -1, 1, 1)


def _params(flat, w, is_fc, dtype):
    """float32 parameters as given (the nets' values), widened to `dtype` when that is wider"""
    return {k: v.astype(dtype) for k, v in wts.split_params(np.asarray(flat, np.float32), w, is_fc).items()}


def fc_forward(flat, w, ctx, dtype=np.float32):
    t = _params(flat, w, True, dtype)
    x = _t(np.asarray(ctx, np.float32).reshape(-1, 5 * w * w), dtype)
    for i in range(4):
        x = x @ torch.from_numpy(t["fully_connected/weights_%d" % i]) + torch.from_numpy(t["fully_connected/biases_%d" % i])
        if i < 3:
            x = _leaky(x)
    return x.reshape(-1, w, w).numpy()


def conv_forward(flat, w, above, left, dtype=np.float32):
    t = _params(flat, w, False, dtype)
    st = wts.STRIDES_BRANCH[w]
    feats = []
    for name, inp, shape in (("branch_above", above, (w, 3 * w)), ("branch_left", left, (2 * w, w))):
        x = _t(np.asarray(inp, np.float32).reshape(-1, 1, *shape), dtype)
        for i, s in enumerate(st):
            p = "convolutional/%s/convolution_%d/" % (name, i)
            x = _leaky(_conv_same(x, t[p + "weights"], t[p + "biases"], s))
        feats.append(x)                                                  # [N, C, 4, 12] / [N, C, 8, 4]
    a, l = feats
    n, c = a.shape[0], a.shape[1]
    v = torch.cat([a.reshape(n, c, 48), l.reshape(n, c, 32)], dim=2)     # per channel: [above row-major | left]
    m = "convolutional/merger/"
    Wm = torch.from_numpy(t[m + "channelwise_fully_connected_merger/weights"])   # [C, 80, 16]
    bm = torch.from_numpy(t[m + "channelwise_fully_connected_merger/biases"])    # [C, 16]
    o = torch.einsum("ncp,cpj->ncj", v, Wm) + bm.unsqueeze(0)
    x = _leaky(o).reshape(n, c, 4, 4)
    rev = st[::-1]
    for i, s in enumerate(rev):
        p = m + "transpose_convolution_%d/" % i
        x = _tconv_same(x, t[p + "weights"], t[p + "biases"], s)
        if i != len(rev) - 1:
            x = _leaky(x)
    return x.reshape(n, w, w).numpy()
