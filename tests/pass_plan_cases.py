"""The case table of the pass layer's plan (csrc/pnn_passes.cpp): the smallest shapes at which each of its launch paths is taken, on the
seeded nets of util.make_params.  One table for tests/test_gpu_pass_plan.py (the statistics of every case against recorded triples) and
tools/lib_ab_plan.py (outputs, [pnn] lines and statistics of two builds against each other).  Every case runs in a context of its own
with "autotune" = 0: a timed sweep would make the plan depend on the clock."""
import functools

import numpy as np

from tests import util

P1 = (("precision", 1),)


def _case(name, fc, w, n, opts=(), mode="host"):
    return (name, fc, w, n, tuple(opts), mode)


CASES = (
    # FC, exact f32: chain order + inline host rows + one-launch output layer (1, 5); past the 512 blocks of that output layer and the
    # small kernels' tile cap: fc_out_f32 + fuse_reduce behind the fcseg tiles (600); the fused output layer (1024)
    [_case("fc%d_%d" % (w, n), True, w, n) for w in (4, 8) for n in (1, 5, 600, 1024)]
    # conv, exact f32: pair path, merger tail, last-layer tail, folded K segments at 32 / 64
    + [_case("conv%d_%d" % (w, n), False, w, n) for w in (4, 8, 16, 32, 64) for n in (1, 5)]
    # ... and twice in one context: the second pass overlaps its branches on two streams
    + [_case("conv16_256_twice", False, 16, 256, mode="twice")]
    # split f16: small kernel, K-segment output layer, ring fusion; the pair path and the image kernel with first and last layer delegated
    + [_case("fc8_%d_sp" % n, True, 8, n, P1) for n in (1, 5, 1024)]
    + [_case("conv16_%d_sp" % n, False, 16, n, P1) for n in (1, 200)]
    # conv 32 x 32 at one block, each option against conv32_1
    + [_case("conv32_1_%s0" % o, False, 32, 1, ((o, 0),)) for o in ("pair", "tails", "chain_io", "seg_fold")]
    + [_case("conv32_1_two_streams", False, 32, 1, (("branch_streams", 2), ("pair", 0))),
       _case("conv32_1_timed", False, 32, 1, (("time_launches", 1),)),
       _case("conv32_70_seq", False, 32, 70, (("f32_seg_mode", 1),))]
    # the chunk loop: every chunk carries its host rows, the last one the done signal
    + [_case("fc8_5_chunk3", True, 8, 5, (("max_chunk", 3),)), _case("conv16_5_chunk3", False, 16, 5, (("max_chunk", 3),))]
    # pnn_predict_tbs_device, the first convolutions reading the picture plane: pair and layer-by-layer form, both arithmetics
    + [_case("conv16_tbs_%d%s" % (n, "_sp" if o else ""), False, 16, n, o, "tbs") for o in ((), P1) for n in (2, 200)]
)
NAMES = [c[0] for c in CASES]


@functools.lru_cache(maxsize=None)
def _params(w, fc):
    return util.make_params(w, fc, 7, out_gain=util.out_gain(w, fc))


def _tbs_call(net, w, n):
    import ctypes
    import torch
    from context_adaptive_neural_network_based_prediction_amd import _lib
    L = _lib.lib()
    plane = util.make_plane(288, 448, seed=9, pad=16)
    xs, ys, flags = util.make_tbs(288, 448, w, n, seed=10, partial_fraction=0.5)
    units = 2 * w // 4
    arr = (_lib.TbDev * n)()
    for i in range(n):
        assert L.pnn_make_tb_desc(ctypes.byref(arr[i]), int(ys[i]) * plane.shape[1] + int(xs[i]), plane.shape[1],
                                  flags[i].ctypes.data_as(_lib.u8p), int(flags[i].sum()), units, units) == 0
    d_plane, d_tbs = util.dev(plane), util.dev(np.frombuffer(arr, dtype=np.uint8).copy())
    d_dst = torch.full((n, w, w), -1, dtype=torch.int32, device="cuda")
    d_f32 = torch.full((n, w, w), float("nan"), dtype=torch.float32, device="cuda")
    rc = L.pnn_predict_tbs_device(net.ctx, w, d_plane.data_ptr(), 4, d_tbs.data_ptr(), n, d_dst.data_ptr(), d_f32.data_ptr(), None)
    assert rc == 0, L.pnn_last_error(net.ctx)
    torch.cuda.synchronize()
    return np.concatenate([d_f32.cpu().numpy().ravel(), d_dst.cpu().numpy().ravel().astype(np.float32)])


def run_case(case):
    """-> (the case's float32 output, (launches, gemm_launches, gemm_flops) of its last call)."""
    from context_adaptive_neural_network_based_prediction_amd import PredictionNeuralNetwork
    _, fc, w, n, opts, mode = case
    net = PredictionNeuralNetwork(n, w, fc, params=_params(w, fc))
    net.set_option("autotune", 0)
    for k, v in opts:
        net.set_option(k, v)
    if mode == "tbs":
        out = _tbs_call(net, w, n)
    else:
        a, l = util.make_contexts(w, n, 8)
        ins = (util.flatten_fc(a, l),) if fc else (a, l)
        for _ in range(2 if mode == "twice" else 1):
            out = net.predict(*ins)
    st = net.last_call_stats()
    net.close()
    return np.asarray(out, np.float32), (st["launches"], st["gemm_launches"], st["gemm_flops"])
