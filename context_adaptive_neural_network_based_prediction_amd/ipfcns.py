"""IPFCN-S, the evaluator's second competitor, mirroring the reference's ipfcns/ipfcns.py (extract_pair(s)_groups_lines_from_
channel(s)[_plus_preprocessing], preprocess_pairs_groups_lines, predict_by_batch_via_ipfcns): same names, arguments, return
dtypes and shapes, same exceptions for bad arguments.  Caffe is not needed: the net is four InnerProduct layers with PReLU between
them (IntraFCN205_deploy_Size{4,8,16,32}.prototxt), run by libpnn_hip.so on the GPU (NetIpfcns) in the exact-f32 order of
INTEGRATION.md section 4, with a bit-identical host twin (forward_host).  read_caffemodel decodes a trained .caffemodel without
Caffe or protobuf.

Preprocessing keeps the reference's float32 semantics of the numpy-1 era it was written for: S, the sum of the K = 64 + 32 w
samples, is an integer (exact in float32), mean = fl32(S / K) correctly rounded, x = fl32(p - mean).  (numpy >= 2 promotes the
reference's `float32 sum / int64 size` to float64; the float32 form is the one kept here, on the host and on the GPU alike.)
"""
import ctypes
import struct

import numpy as np

from . import _lib

WIDTHS = (4, 8, 16, 32)
HIDDEN = {4: 512, 8: 1024, 16: 1024, 32: 2048}
LAYER_NAMES = ('fc1', 'relu1', 'fc2', 'relu2', 'fc3', 'relu3', 'fc4')


def input_size(width_target):
    return 64 + 32 * width_target


def layer_dims(width_target):
    """(K, H, w^2) of the width's IPFCN-S."""
    if width_target not in WIDTHS:
        raise ValueError('There is no IPFCN-S for `width_target` = %r (4, 8, 16 or 32).' % (width_target,))
    return input_size(width_target), HIDDEN[width_target], width_target * width_target


def n_params(width_target):
    K, H, O = layer_dims(width_target)
    return H * K + 2 * H + 2 * (H * H + 2 * H) + O * H + O


def _check_lines_position(height_channel, width_channel, width_target, row_1st, col_1st):
    if width_target < 0:
        raise ValueError('`width_target` is not positive.')
    if row_1st < 0:
        raise ValueError('`row_1st` is not positive.')
    if col_1st < 0:
        raise ValueError('`col_1st` is not positive.')
    if row_1st + 2 * width_target + 8 > height_channel:
        raise ValueError('`row_1st + 2*width_target + 8` is not smaller than `channel_single_or_pair_uint8.shape[0]`.')
    if col_1st + 2 * width_target + 8 > width_channel:
        raise ValueError('`col_1st + 2*width_target + 8` is not smaller than `channel_single_or_pair_uint8.shape[1]`.')


def extract_pair_groups_lines_from_channel(channel_single_or_pair_uint8, width_target, row_1st, col_1st):
    """ipfcns.py:97-191: (above group [8, 2w+8, 1], left group [2w, 8, 1]) uint8 of the line origin (row_1st, col_1st); with two
    channels the second (the compressed one) is read."""
    if channel_single_or_pair_uint8.dtype != np.uint8:
        raise TypeError('`channel_single_or_pair_uint8.dtype` is not equal to `numpy.uint8`.')
    (height_channel, width_channel, nb_channels) = channel_single_or_pair_uint8.shape
    _check_lines_position(height_channel, width_channel, width_target, row_1st, col_1st)
    if nb_channels in (1, 2):
        i = nb_channels - 1
    else:
        raise ValueError('`channel_single_or_pair_uint8.shape[2]` does not belong to {1, 2}.')
    above = channel_single_or_pair_uint8[row_1st:row_1st + 8, col_1st:col_1st + 2 * width_target + 8, i:i + 1]
    left = channel_single_or_pair_uint8[row_1st + 8:row_1st + 2 * width_target + 8, col_1st:col_1st + 8, i:i + 1]
    return (above, left)


def _check_origins(row_1sts, col_1sts):
    if not np.issubdtype(row_1sts.dtype, np.integer):
        raise TypeError('`row_1sts.dtype` is not smaller than `numpy.integer` in type hierarchy.')
    if not np.issubdtype(col_1sts.dtype, np.integer):
        raise TypeError('`col_1sts.dtype` is not smaller than `numpy.integer` in type hierarchy.')
    if col_1sts.size != row_1sts.size:
        raise ValueError('`col_1sts.size` is not equal to `row_1sts.size`.')
    if row_1sts.ndim != 1 or col_1sts.ndim != 1:
        raise ValueError('can only convert an array of size 1 to a Python scalar')


def extract_pairs_groups_lines_from_channels(channels_single_or_pair_uint8, width_target, row_1sts, col_1sts):
    """ipfcns.py:276-335, vectorised: (above groups [images*positions, 8, 2w+8, 1], left groups [images*positions, 2w, 8, 1]),
    uint8, image-major."""
    _check_origins(row_1sts, col_1sts)
    nb_images, n = channels_single_or_pair_uint8.shape[0], row_1sts.size
    above = np.zeros((nb_images * n, 8, 2 * width_target + 8, 1), dtype=np.uint8)
    left = np.zeros((nb_images * n, 2 * width_target, 8, 1), dtype=np.uint8)
    if nb_images == 0 or n == 0:
        return (above, left)
    if channels_single_or_pair_uint8.dtype != np.uint8:
        raise TypeError('`channel_single_or_pair_uint8.dtype` is not equal to `numpy.uint8`.')
    if channels_single_or_pair_uint8.ndim != 4:
        raise ValueError('not enough values to unpack (expected 3)')
    (_, height_channel, width_channel, nb_channels) = channels_single_or_pair_uint8.shape
    rows, cols = row_1sts.astype(np.int64), col_1sts.astype(np.int64)
    _check_lines_position(height_channel, width_channel, width_target, int(rows.min()), int(cols.min()))
    _check_lines_position(height_channel, width_channel, width_target, int(rows.max()), int(cols.max()))
    if nb_channels not in (1, 2):
        raise ValueError('`channel_single_or_pair_uint8.shape[2]` does not belong to {1, 2}.')
    ch = channels_single_or_pair_uint8[:, :, :, nb_channels - 1]
    ra, ca = np.arange(8), np.arange(2 * width_target + 8)
    above[:, :, :, 0] = ch[:, rows[:, None, None] + ra[None, :, None], cols[:, None, None] + ca[None, None, :]].reshape(
        nb_images * n, 8, 2 * width_target + 8)
    rl, cl = 8 + np.arange(2 * width_target), np.arange(8)
    left[:, :, :, 0] = ch[:, rows[:, None, None] + rl[None, :, None], cols[:, None, None] + cl[None, None, :]].reshape(
        nb_images * n, 2 * width_target, 8)
    return (above, left)


def extract_pairs_groups_lines_from_channel(channel_single_or_pair_uint8, width_target, row_1sts, col_1sts):
    """ipfcns.py:193-274, vectorised: the groups of every line origin of one image channel."""
    if channel_single_or_pair_uint8.dtype != np.uint8:
        raise TypeError('`channel_single_or_pair_uint8.dtype` is not equal to `numpy.uint8`.')
    if channel_single_or_pair_uint8.ndim != 3:
        raise ValueError('not enough values to unpack (expected 3)')
    return extract_pairs_groups_lines_from_channels(channel_single_or_pair_uint8[None], width_target, row_1sts, col_1sts)


def preprocess_pairs_groups_lines(groups_lines_above_uint8, groups_lines_left_uint8):
    """ipfcns.py:432-494 with the pinned float32 semantics (module docstring): (flattened pairs [N, 64 + 32 w] float32,
    means [N] float32)."""
    n = groups_lines_above_uint8.shape[0]
    flat = np.concatenate((groups_lines_above_uint8.reshape(n, -1), groups_lines_left_uint8.reshape(n, -1)), axis=1)
    size_group = flat.shape[1]
    sums = flat.astype(np.int64).sum(axis=1)
    means_float32 = sums.astype(np.float32) / np.float32(size_group)
    flattened = flat.astype(np.float32) - means_float32[:, None]
    return (flattened.astype(np.float32), means_float32.astype(np.float32))


def extract_pairs_groups_lines_from_channels_plus_preprocessing(channels_single_or_pair_uint8, width_target, row_1sts, col_1sts):
    """ipfcns.py:337-386."""
    (above, left) = extract_pairs_groups_lines_from_channels(channels_single_or_pair_uint8, width_target, row_1sts, col_1sts)
    return preprocess_pairs_groups_lines(above, left)


# ---- weights ----------------------------------------------------------------------------------------------------------------

def _varint(buf, pos):
    result = shift = 0
    while True:
        if pos >= len(buf):
            raise ValueError('truncated varint in the caffemodel')
        b = buf[pos]
        pos += 1
        result |= (b & 0x7f) << shift
        if not b & 0x80:
            return result, pos
        shift += 7
        if shift > 63:
            raise ValueError('varint longer than 10 bytes in the caffemodel')


def _fields(buf):
    """(field number, wire type, value) of a protobuf message; value = int (varint, fixed) or bytes (length-delimited)."""
    pos = 0
    while pos < len(buf):
        key, pos = _varint(buf, pos)
        field, wt = key >> 3, key & 7
        if wt == 0:
            v, pos = _varint(buf, pos)
        elif wt == 1:
            if pos + 8 > len(buf):
                raise ValueError('truncated fixed64 in the caffemodel')
            v, pos = buf[pos:pos + 8], pos + 8
        elif wt == 2:
            ln, pos = _varint(buf, pos)
            if pos + ln > len(buf):
                raise ValueError('truncated length-delimited field in the caffemodel')
            v, pos = buf[pos:pos + ln], pos + ln
        elif wt == 5:
            if pos + 4 > len(buf):
                raise ValueError('truncated fixed32 in the caffemodel')
            v, pos = buf[pos:pos + 4], pos + 4
        else:
            raise ValueError('unsupported wire type %d in the caffemodel' % wt)
        yield field, wt, v


def _blob(buf):
    """BlobProto: data = 5 (packed or not), shape = 7 (BlobShape.dim = 1), legacy num / channels / height / width = 1 .. 4."""
    data, dims, legacy = [], None, [None] * 4
    for field, wt, v in _fields(buf):
        if field == 5:
            if wt == 2:
                if len(v) % 4:
                    raise ValueError('packed float data of %d bytes' % len(v))
                data.append(np.frombuffer(bytes(v), dtype='<f4'))
            elif wt == 5:
                data.append(np.frombuffer(bytes(v), dtype='<f4'))
            else:
                raise ValueError('BlobProto.data with wire type %d' % wt)
        elif field == 7 and wt == 2:
            dims = []
            for f2, wt2, v2 in _fields(v):
                if f2 != 1:
                    continue
                if wt2 == 0:
                    dims.append(v2)
                elif wt2 == 2:
                    p = 0
                    while p < len(v2):
                        d, p = _varint(v2, p)
                        dims.append(d)
                else:
                    raise ValueError('BlobShape.dim with wire type %d' % wt2)
        elif 1 <= field <= 4 and wt == 0:
            legacy[field - 1] = v
    values = np.concatenate(data) if data else np.zeros(0, dtype='<f4')
    if dims is None:
        dims = [1 if d is None else d for d in legacy] if any(d is not None for d in legacy) else [values.size]
    if int(np.prod(dims, dtype=np.int64)) != values.size:
        raise ValueError('a blob of shape %s holds %d values' % (tuple(dims), values.size))
    return values.astype(np.float32).reshape(dims)


def read_caffemodel(path):
    """Decodes a Caffe NetParameter file (layer = 100; LayerParameter name = 1, type = 2, blobs = 7) without Caffe or protobuf:
    a list of (name, type, [blobs as float32 arrays in their stored shape]), in file order.  Refuses V1 files (`layers` = 2),
    truncated messages and blobs whose value count does not match their shape (ValueError)."""
    with open(path, 'rb') as f:
        buf = f.read()
    layers = []
    for field, wt, v in _fields(buf):
        if field == 2 and wt == 2:
            raise ValueError('%s is a V1 caffemodel (`layers`, field 2): upgrade it to `layer`' % path)
        if field != 100 or wt != 2:
            continue
        name, kind, blobs = '', '', []
        for f2, wt2, v2 in _fields(v):
            if f2 == 1 and wt2 == 2:
                name = bytes(v2).decode()
            elif f2 == 2 and wt2 == 2:
                kind = bytes(v2).decode()
            elif f2 == 7 and wt2 == 2:
                blobs.append(_blob(v2))
        layers.append((name, kind, blobs))
    return layers


def params_from_caffemodel(layers, width_target):
    """The canonical flat parameters (W1[H][K], b1, a1, W2, b2, a2, W3, b3, a3, W4[w^2][H], b4) from read_caffemodel's list;
    ValueError for a missing layer, a missing blob or one of the wrong shape."""
    K, H, O = layer_dims(width_target)
    by_name = {name: blobs for (name, _, blobs) in layers}
    want = {'fc1': [(H, K), (H,)], 'relu1': [(H,)], 'fc2': [(H, H), (H,)], 'relu2': [(H,)],
            'fc3': [(H, H), (H,)], 'relu3': [(H,)], 'fc4': [(O, H), (O,)]}
    out = []
    for name in LAYER_NAMES:
        if name not in by_name:
            raise ValueError('the caffemodel has no layer `%s`' % name)
        blobs = by_name[name]
        if len(blobs) != len(want[name]):
            raise ValueError('layer `%s` has %d blobs, IPFCN-S needs %d' % (name, len(blobs), len(want[name])))
        for blob, shape in zip(blobs, want[name]):
            squeezed = tuple(d for d in blob.shape if d != 1) or (1,)
            if squeezed != tuple(d for d in shape if d != 1) or blob.size != int(np.prod(shape)):
                raise ValueError('blob of layer `%s` has shape %s, expected %s' % (name, blob.shape, shape))
            out.append(blob.reshape(-1))
    return np.ascontiguousarray(np.concatenate(out).astype(np.float32))


# ---- the net ----------------------------------------------------------------------------------------------------------------

def forward_host(params, width_target, flattened_float32, layers=4):
    """The host twin (pnn_ipfcns_forward_host): the activations after layer `layers` (1 .. 3: [N, H] behind the PReLU; 4: fc4
    [N, w^2], without the mean), bit-identical to the GPU pass."""
    K, H, O = layer_dims(width_target)
    params = np.ascontiguousarray(params, dtype=np.float32)
    if params.size != n_params(width_target):
        raise ValueError('%d parameters given, the width-%d IPFCN-S needs %d' % (params.size, width_target, n_params(width_target)))
    x = np.ascontiguousarray(flattened_float32, dtype=np.float32)
    if x.ndim != 2 or x.shape[1] != K:
        raise ValueError('the flattened pairs must be [N, %d]' % K)
    out = np.zeros((x.shape[0], O if layers == 4 else H), dtype=np.float32)
    rc = _lib.lib().pnn_ipfcns_forward_host(width_target, params.ctypes.data_as(_lib.f32p), x.ctypes.data_as(_lib.f32p),
                                            x.shape[0], layers, out.ctypes.data_as(_lib.f32p))
    if rc != 0:
        raise ValueError('pnn_ipfcns_forward_host refused the arguments (width %d, layers %d)' % (width_target, layers))
    return out


class NetIpfcns:
    """The IPFCN-S of one width on a model-less context of `device` (stands in for the reference's caffe.Net)."""

    def __init__(self, width_target, params, device=0):
        import torch                                      # noqa: F401  (one HIP runtime with torch, see _lib)
        layer_dims(width_target)
        self.width_target = width_target
        self.device = device
        L = _lib.lib()
        self.ctx = ctypes.c_void_p()
        _lib.check(L.pnn_create_empty(ctypes.byref(self.ctx), ctypes.c_float(0.), device))
        self.load(params)

    @classmethod
    def from_caffemodel(cls, path, width_target, device=0):
        return cls(width_target, params_from_caffemodel(read_caffemodel(path), width_target), device)

    def load(self, params):
        params = np.ascontiguousarray(params, dtype=np.float32).reshape(-1)
        _lib.check(_lib.lib().pnn_ipfcns_load(self.ctx, self.width_target, params.ctypes.data_as(_lib.f32p), params.size), self.ctx)

    def set_option(self, name, value):
        _lib.check(_lib.lib().pnn_set_option(self.ctx, name.encode(), int(value)), self.ctx)

    def _stream(self):
        import torch
        return torch.cuda.current_stream(torch.device('cuda', self.device))

    def forward_device(self, d_x):
        """fc4 [N, w^2] float32 torch tensor on the device from the flattened pairs d_x [N, K] (a float32 torch tensor there)."""
        import torch
        n = d_x.shape[0]
        out = torch.empty((n, self.width_target ** 2), dtype=torch.float32, device=d_x.device)
        s = self._stream()
        with torch.cuda.device(d_x.device):
            _lib.check(_lib.lib().pnn_ipfcns_forward_device(self.ctx, self.width_target, d_x.data_ptr(), n, out.data_ptr(),
                                                            ctypes.c_void_p(s.cuda_stream)), self.ctx)
        s.synchronize()
        return out

    def forward(self, flattened_float32):
        import torch
        x = torch.from_numpy(np.ascontiguousarray(flattened_float32, dtype=np.float32)).to(torch.device('cuda', self.device))
        return self.forward_device(x).cpu().numpy()

    def predict_from_channels_device(self, d_channels, d_rows, d_cols, d_targets=None, pred_u8=True, pred_f32=False, means=False):
        """The fused GPU path (pnn_ipfcns_predict_device) on torch tensors already on the device: channels uint8 [images, H, W],
        line origins int32 [positions].  Returns (uint8 [n, w, w] or None, float32 [n, w, w] or None, means [n] or None, SSE
        uint32 as int64 [n] or None), n = images x positions, image-major."""
        import torch
        images, height, width_ch = d_channels.shape
        positions = d_rows.shape[0]
        n, w = images * positions, self.width_target
        dev = d_channels.device
        u8 = torch.empty((n, w, w), dtype=torch.uint8, device=dev) if pred_u8 else None
        f32 = torch.empty((n, w, w), dtype=torch.float32, device=dev) if pred_f32 else None
        mn = torch.empty(n, dtype=torch.float32, device=dev) if means else None
        sse = torch.empty(n, dtype=torch.int32, device=dev) if d_targets is not None else None
        s = self._stream()
        ptr = (lambda t: t.data_ptr() if t is not None else None)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().pnn_ipfcns_predict_device(
                self.ctx, w, d_channels.data_ptr(), images, height, width_ch, d_rows.data_ptr(), d_cols.data_ptr(), positions,
                ptr(d_targets), ptr(u8), ptr(f32), ptr(mn), ptr(sse), ctypes.c_void_p(s.cuda_stream)), self.ctx)
        s.synchronize()
        sse_out = None if sse is None else sse.cpu().numpy().view(np.uint32).astype(np.int64)
        return (None if u8 is None else u8.cpu().numpy(), None if f32 is None else f32.cpu().numpy(),
                None if mn is None else mn.cpu().numpy(), sse_out)

    def close(self):
        if self.ctx:
            _lib.lib().pnn_destroy(self.ctx)
            self.ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def predict_by_batch_via_ipfcns(flattened_pairs_groups_lines_float32, net_ipfcns, width_target, batch_size):
    """ipfcns.py:388-430: fc4 of every row as [N, w, w, 1] float32 (without the mean).  The batches only bound what the
    reference's net held at once; the predictions do not depend on them, so the whole array goes to the GPU in one call."""
    nb_predictions = flattened_pairs_groups_lines_float32.shape[0]
    if nb_predictions % batch_size:
        raise ValueError('`numerator` is not divisible by `denominator`.')
    if net_ipfcns.width_target != width_target:
        raise ValueError('the net is the width-%d IPFCN-S, not the width-%d one' % (net_ipfcns.width_target, width_target))
    if nb_predictions == 0:
        return np.zeros((0, width_target, width_target, 1), dtype=np.float32)
    return net_ipfcns.forward(flattened_pairs_groups_lines_float32).reshape(nb_predictions, width_target, width_target, 1)
