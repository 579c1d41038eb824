"""What the coding tree over a whole picture costs, on one box (writes profiles/cu_tree_picture.txt anew):

  pnn_cu_tree_picture_device on synthetic device leaves for a grid of 17 x 30 CTUs (a 1920 x 1080 picture's, rounded up to whole
  CTUs), 1 image, 4 QPs -- 46 launches, one per anti-diagonal -- beside the unchanged pnn_cu_tree_device on the same 510 CTUs with
  edges absent: one launch, the only baseline there is.  The entries alternate in one process; a sample is `--calls` back-to-back
  calls of one entry between two HIP events on the stream, the median and min .. max of `--reps` samples (at least 20) after
  `--warmup` ones count.  Before anything is timed the picture entry's outputs are compared with the host twin.  The walk's bound is
  NOT found here: that needs a counter run, collected in a run of its own.

  Then the evaluator on the 256 x 256 test picture of tests/test_gpu_cu_tree_picture_evaluator.py (2 x 2 CTUs, QPs 22 and 37, the
  switch codec): evaluation.coding_tree_from_pictures beside the five score calls + evaluation.coding_tree_from_scores, wall clock
  around each after a synchronize (median of `--evaluator-reps`), and the bytes each moves over PCIe for leaves and results, counted
  from the layouts.

    python tools/cu_tree_picture_rate.py         # on the GPU box
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from hevc_mode_hads_rate import sample  # noqa: E402

ROWS, COLS, QPS = 17, 30, (22, 27, 32, 37)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--calls", type=int, default=5, help="back-to-back calls per timed sample")
    ap.add_argument("--evaluator-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cu_tree_picture.txt"))
    args = ap.parse_args()
    assert args.reps >= 20, "at least 20 timed samples"
    import torch
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    from context_adaptive_neural_network_based_prediction_amd import _lib, evaluation
    from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
    from tests import cu_tree_cases as cc
    from tests import cu_tree_picture_cases as pc
    from tests import util
    L = _lib.lib()
    ctx = ip._context(0)
    s = torch.cuda.current_stream()
    sp = ctypes.c_void_p(s.cuda_stream)
    nq, n_ctu = len(QPS), ROWS * COLS
    c_qps = (ctypes.c_int * nq)(*QPS)
    pointers = ctypes.c_void_p * 5
    leaves = pc.near_tie_leaves(n_ctu, QPS, None, 17)
    held = {w: [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a.view(np.int64) if a.dtype == np.uint64 else a).cuda()
                for a in leaves[w]] for w in ip.WIDTHS}
    tables = [pointers(*[held[w][k].data_ptr() for w in ip.WIDTHS]) for k in range(3)]
    shapes = ip.cu_tree_picture_shapes(nq, 1, ROWS, COLS)
    outs = [torch.zeros(max(int(np.prod(shape)) * np.dtype(dtype).itemsize, 8), dtype=torch.uint8, device="cuda")
            for (_, dtype), shape in zip(ip.CU_TREE_PICTURE_OUTPUTS, shapes)]
    nb_ws = L.pnn_cu_tree_picture_workspace_bytes(nq, 1, ROWS, COLS)
    d_ws = torch.empty(nb_ws, dtype=torch.uint8, device="cuda")

    def picture():
        return L.pnn_cu_tree_picture_device(ctx, c_qps, nq, None, 1, ROWS, COLS, *tables, 35, *[o.data_ptr() for o in outs], d_ws.data_ptr(), nb_ws, sp)

    def unchained():
        return L.pnn_cu_tree_device(ctx, c_qps, nq, None, n_ctu, *tables, None, None, 35, *[o.data_ptr() for o in outs[:8]], sp)

    def launches():
        count = ctypes.c_int(-1)
        assert L.pnn_last_call_stats(ctx, None, None, ctypes.byref(count)) == 0
        return count.value

    assert picture() == 0
    torch.cuda.synchronize()
    launches_picture = launches()
    host = ip.cu_tree_picture(cc.as_rd_pass_tuples(leaves), QPS, 1, ROWS, COLS)
    for (name, dtype), shape, d_o in zip(ip.CU_TREE_PICTURE_OUTPUTS, shapes, outs):
        got = d_o.cpu().numpy()[:int(np.prod(shape)) * np.dtype(dtype).itemsize].view(dtype).reshape(shape)
        want = (host["image_rate_bits"] * 32768.).astype(np.uint64) if name == "image_rates" else host[name]
        assert got.tobytes() == want.tobytes(), "%s differs from the host twin" % name
    assert unchained() == 0
    torch.cuda.synchronize()
    launches_unchained = launches()
    moved = int((outs[0].cpu().numpy()[:nq * n_ctu * 64].reshape(nq, n_ctu, 64) != host["cu_depths"]).any(axis=2).sum())

    calls = {"picture": picture, "unchained": unchained}
    times = {name: [] for name in calls}
    for i in range(args.warmup + args.reps):
        for name in (list(calls)[::-1] if i % 2 else list(calls)):
            t = sample(torch, s, calls[name], args.calls)
            if i >= args.warmup:
                times[name].append(t)
    med = {name: statistics.median(v) for name, v in times.items()}
    fmt = lambda name: "%.1f [%.1f .. %.1f]" % (med[name], min(times[name]), max(times[name]))

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        def out(line):
            print(line, flush=True)
            f.write(line + "\n")
        props = torch.cuda.get_device_properties(0)
        out("# tools/cu_tree_picture_rate.py on one GPU of architecture %s, %d compute units (torch names it \"%s\"): %d warm-up + %d timed"
            % (props.gcnArchName, props.multi_processor_count, torch.cuda.get_device_name(0), args.warmup, args.reps))
        out("# samples of %d back-to-back calls between two HIP events on the" % args.calls)
        out("# stream, entries alternating; us per call, median [min .. max]; %d x %d CTUs, 1 image, %d QPs %s, synthetic near-tie leaves" % (ROWS, COLS, nq, QPS))
        out("pnn_cu_tree_picture_device  %s  %d launches (%.1f us per launch)" % (fmt("picture"), launches_picture, med["picture"] / launches_picture))
        out("pnn_cu_tree_device          %s  %d launch, edges absent (the parent's code)" % (fmt("unchained"), launches_unchained))
        out("chained / unchained = %.1f; %d of the %d (QP, CTU) maps differ between the two" % (med["picture"] / med["unchained"], moved, nq * n_ctu))

        # the evaluator on the test picture
        channels = pc.evaluator_channels(False, pc.SEEDS['switch'])
        nets = {w: util.make_net(w, w <= 8, pc.POSITIONS[w][0].size) for w in ip.WIDTHS}
        means = dict.fromkeys(ip.WIDTHS, util.MEAN)
        options = dict(pc.OPTIONS, keep_predictions=False, first_pass=True, transform_qps=pc.EVALUATOR_QPS, rd_pass=True, rd_pass_signalling=True)

        def from_pictures():
            return evaluation.coding_tree_from_pictures(channels, nets, means, pc.ROW_1ST, pc.COL_1ST, pc.CTU_ROWS, pc.CTU_COLS, pc.EVALUATOR_QPS, **pc.OPTIONS)

        def through_the_host():
            scores = {w: evaluation.score_masks_from_pictures(channels, w, pc.POSITIONS[w][0], pc.POSITIONS[w][1], nets[w], util.MEAN, ((0, 0),), **options)
                      for w in ip.WIDTHS}
            return evaluation.coding_tree_from_scores(scores, device=0)

        try:
            wall = {"from_pictures": [], "through_the_host": []}
            for i in range(1 + args.evaluator_reps):
                for name, call in (("from_pictures", from_pictures), ("through_the_host", through_the_host)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    call()
                    torch.cuda.synchronize()
                    if i:
                        wall[name].append((time.perf_counter() - t0) * 1e3)
        finally:
            for net in nets.values():
                net.close()
        nq2, ctus = len(pc.EVALUATOR_QPS), pc.CTU_ROWS * pc.CTU_COLS
        blocks = sum(ctus * (64 // w) ** 2 for w in ip.WIDTHS)
        down_scores = sum(evaluation._output_layout(ctus * (64 // w) ** 2, w, True, nq2, True, True, True)[1]['predictions_pnn'] for w in ip.WIDTHS)
        tree_down = sum(int(np.prod(shape)) * np.dtype(dtype).itemsize
                        for (_, dtype), shape in zip(ip.CU_TREE_PICTURE_OUTPUTS, ip.cu_tree_picture_shapes(nq2, 1, pc.CTU_ROWS, pc.CTU_COLS)))
        tree_down_old = sum(int(np.prod(shape)) * np.dtype(dtype).itemsize
                            for (_, dtype), shape in zip(ip.CU_TREE_OUTPUTS, ip.cu_tree_shapes(nq2, ctus)))
        out("# evaluator, 256 x 256 picture, 2 x 2 CTUs, QPs %s, switch codec: wall clock in ms, median [min .. max] of %d calls after one" % (pc.EVALUATOR_QPS, args.evaluator_reps))
        for name in wall:
            out("%-18s %.1f [%.1f .. %.1f]" % (name, statistics.median(wall[name]), min(wall[name]), max(wall[name])))
        up_both = sum(channels.nbytes + 2 * 4 * pc.POSITIONS[w][0].size for w in ip.WIDTHS)
        out("PCIe.  Both upload the picture and the int32 positions once per width, %d bytes over the five widths.  Beside that," % up_both)
        out("coding_tree_from_pictures downloads %d bytes (the tree's outputs) and uploads no leaves;" % tree_down)
        out("the chain downloads %d bytes of score results, uploads %d bytes of leaves (%d blocks x %d QPs x 13 bytes: dist, rate, mode) and downloads %d"
            % (down_scores, blocks * nq2 * 13, blocks, nq2, tree_down_old))


if __name__ == "__main__":
    main()
