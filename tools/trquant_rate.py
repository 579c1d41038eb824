"""What the open-loop transform coding costs, on one box (writes profiles/trquant_rate.txt):

  trquant_kernel (pnn_trquant_device: forward transform once, then quantisation, dequantisation, inverse transform, reconstruction and the
  three sums per QP, at 4 QPs) on dense blocks, w = 8 with N = 65 536 and w = 32 with N = 8 192, next to hevc_best_mode_kernel
  (pnn_hevc_best_mode_device: index + SSE) on blocks of the same sizes in the same run, as a size reference: the evaluator makes two
  transform-coding calls behind every search.  The two alternate in one process; a sample is `--calls` back-to-back calls of one entry
  between two HIP events, the median of `--reps` samples after `--warmup` ones counts (the method of tools/hevc_mode_hads_rate.py).
  Before anything is timed every output of the kernel, reconstructions included, is compared with the host twin on the first blocks:
  faster and different is not faster.

    python tools/trquant_rate.py           # on the GPU box
"""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from hevc_mode_hads_rate import blocks, sample  # noqa: E402

SHAPES = ((8, 65536), (32, 8192))
QPS = (22, 27, 32, 37)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20, help="back-to-back calls per timed sample")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trquant_rate.txt"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    from context_adaptive_neural_network_based_prediction_amd import _lib
    from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
    L = _lib.lib()
    ctx = ip._context(0)
    s = torch.cuda.current_stream()
    sp = ctypes.c_void_p(s.cuda_stream)
    nq = len(QPS)
    c_qps = (ctypes.c_int * nq)(*QPS)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        def out(line):
            print(line, flush=True)
            f.write(line + "\n")
        out("# tools/trquant_rate.py on one %s: %d warm-up + %d timed samples each, alternating; a sample = %d back-to-back calls between"
            % (torch.cuda.get_device_name(0), args.warmup, args.reps, args.calls))
        out("# two HIP events; us per call (median [min .. max]); TQ = pnn_trquant_device at the %d QPs %s (SSE, nonzero levels, sum of magnitudes;" % (nq, QPS))
        out("# no reconstructions stored), SSE = pnn_hevc_best_mode_device (index + SSE) on blocks of the same size: a size reference")
        out("%-3s %8s %26s %12s %14s %26s %12s" % ("w", "N", "TQ us/call", "blocks/s", "block-QPs/s", "SSE us/call", "x SSE search"))
        for w, n in SHAPES:
            patterns, targets, candidate = blocks(w, n, 50 + w)
            d_p, d_t, d_c = (torch.from_numpy(a).cuda() for a in (patterns, targets, candidate))
            counts = torch.empty((3, nq, n), dtype=torch.int32, device="cuda")
            recon = torch.empty((nq, n, w, w), dtype=torch.uint8, device="cuda")
            index = torch.empty(n, dtype=torch.uint8, device="cuda")
            sse = torch.empty(n, dtype=torch.int32, device="cuda")

            def code(d_recon=None):
                return L.pnn_trquant_device(ctx, w, d_c.data_ptr(), d_t.data_ptr(), n, c_qps, nq, counts[0].data_ptr(), counts[1].data_ptr(),
                                            counts[2].data_ptr(), d_recon, sp)
            calls = {"tq": code,
                     "sse": lambda: L.pnn_hevc_best_mode_device(ctx, w, d_p.data_ptr(), 2 * w + 1, 2 * w + 1, d_t.data_ptr(), n, index.data_ptr(),
                                                                sse.data_ptr(), None, None, sp)}
            # results first
            assert code(recon.data_ptr()) == 0
            torch.cuda.synchronize()
            m = min(n, 256)
            host = ip.transform_code(candidate[:m], targets[:m], QPS, keep_reconstructions=True)
            got = counts[:, :, :m].cpu().numpy().view(np.uint32)
            for k, name in enumerate(("sses_recon", "nb_nonzero_levels", "sum_abs_levels")):
                assert np.array_equal(got[k], host[name]), "w %d: %s differs from the host twin" % (w, name)
            assert np.array_equal(recon[:, :m].cpu().numpy(), host["reconstructions_uint8"]), "w %d: reconstructions differ from the host twin" % w
            times = {name: [] for name in calls}
            for i in range(args.warmup + args.reps):
                for name in calls:
                    t = sample(torch, s, calls[name], args.calls)
                    if i >= args.warmup:
                        times[name].append(t)
            med = {name: statistics.median(v) for name, v in times.items()}
            fmt = lambda name: "%.1f [%.1f .. %.1f]" % (med[name], min(times[name]), max(times[name]))
            out("%-3d %8d %26s %12.4g %14.4g %26s %11.2fx" % (w, n, fmt("tq"), n / med["tq"] * 1e6, n * nq / med["tq"] * 1e6, fmt("sse"),
                                                               med["tq"] / med["sse"]))


if __name__ == "__main__":
    main()
