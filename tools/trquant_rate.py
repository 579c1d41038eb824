"""What the open-loop transform coding costs, on one box (writes profiles/trquant_rate.txt):

  trquant_kernel (pnn_trquant_device: forward transform once, then quantisation, dequantisation, inverse transform, reconstruction and the
  three sums per QP, at 4 QPs) on dense blocks, w = 8 with N = 65 536 and w = 32 with N = 8 192, next to hevc_best_mode_kernel
  (pnn_hevc_best_mode_device: index + SSE) on blocks of the same sizes in the same run, as a size reference: the evaluator makes two
  transform-coding calls behind every search.  The two alternate in one process; a sample is `--calls` back-to-back calls of one entry
  between two HIP events, the median of `--reps` samples after `--warmup` ones counts (the method of tools/hevc_mode_hads_rate.py).
  Before anything is timed every output of the kernel, reconstructions included, is compared with the host twin on the first blocks:
  faster and different is not faster.

  The rate column: pnn_trquant_rate_device with the CABAC rate as a fifth output, without modes (TQ+R) and with
  a mode array that takes every scan (TQ+R modes), in the same alternation, compared with the host twin first, reported as a multiple
  of the no-rate call of the same run.  With --parent-lib, a libpnn_hip.so built from the parent commit joins the alternation (its own
  context, the same buffers): the no-rate call must lie inside the min .. max spread of the parent's samples, or the kernel without
  the rate was disturbed.  The results are APPENDED to profiles/trquant_rate.txt.

  Sign-data hiding: pnn_trquant_sdh_device with the flag set, without the rate (TQ+H) and with it (TQ+R+H), in
  the same alternation, every output compared with the host twin first, each reported as a multiple of the same call without hiding
  (TQ, TQ+R) of the same run; the share of blocks in which hiding changed the reconstruction at some QP is printed beside it.

    python tools/trquant_rate.py [--parent-lib /path/to/parent/libpnn_hip.so]          # on the GPU box
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
    ap.add_argument("--parent-lib", default=None, help="libpnn_hip.so of the parent commit, for the no-rate comparison")
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
    parent = parent_ctx = None
    if args.parent_lib:
        parent = ctypes.CDLL(args.parent_lib)
        parent.pnn_trquant_device.restype, parent.pnn_trquant_device.argtypes = _lib.SIGNATURES["pnn_trquant_device"]
        parent.pnn_create_empty.restype, parent.pnn_create_empty.argtypes = _lib.SIGNATURES["pnn_create_empty"]
        parent_ctx = ctypes.c_void_p()
        assert parent.pnn_create_empty(ctypes.byref(parent_ctx), ctypes.c_float(0.), 0) == 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    legend = "# TQ+R = pnn_trquant_rate_device"
    text = open(args.out).read() if os.path.exists(args.out) else ""
    fresh, known = not text, legend in text               # a file with the legend gets a run line and rows only, an older one the legend too
    with open(args.out, "a") as f:
        def out(line):
            print(line, flush=True)
            f.write(line + "\n")
        if fresh:
            out("# tools/trquant_rate.py on one %s: %d warm-up + %d timed samples each, alternating; a sample = %d back-to-back calls between"
                % (torch.cuda.get_device_name(0), args.warmup, args.reps, args.calls))
            out("# two HIP events; us per call (median [min .. max]); TQ = pnn_trquant_device at the %d QPs %s (SSE, nonzero levels, sum of magnitudes;" % (nq, QPS))
            out("# no reconstructions stored), SSE = pnn_hevc_best_mode_device (index + SSE) on blocks of the same size: a size reference")
        if not known:
            out(legend + ", the same call with the CABAC rate as a fifth output (diagonal scan); TQ+R modes = with a mode")
            out("# array that takes every scan; x TQ = its median over TQ's of this run; parent = pnn_trquant_device of the parent commit's library")
            out("%-3s %8s %26s %12s %14s %26s %12s" % ("w", "N", "TQ us/call", "blocks/s", "block-QPs/s", "SSE us/call", "x SSE search"))
        out("# run: %s, %d warm-up + %d timed samples of %d calls" % (torch.cuda.get_device_name(0), args.warmup, args.reps, args.calls))
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
            bits = torch.empty((nq, n), dtype=torch.int64, device="cuda")
            modes = (np.arange(n) % 35).astype(np.uint8)
            d_modes = torch.from_numpy(modes).cuda()

            def code_rate(d_m=None):
                return L.pnn_trquant_rate_device(ctx, w, d_c.data_ptr(), d_t.data_ptr(), n, d_m, c_qps, nq, counts[0].data_ptr(),
                                                 counts[1].data_ptr(), counts[2].data_ptr(), None, bits.data_ptr(), sp)

            def code_sdh(d_bits=None, d_recon=None):
                return L.pnn_trquant_sdh_device(ctx, w, d_c.data_ptr(), d_t.data_ptr(), n, None, c_qps, nq, counts[0].data_ptr(),
                                                counts[1].data_ptr(), counts[2].data_ptr(), d_recon, d_bits, 1, sp)
            calls = {"tq": code, "tq_sdh": code_sdh, "tq_rate": code_rate, "tq_rate_sdh": lambda: code_sdh(bits.data_ptr()),
                     "tq_rate_modes": lambda: code_rate(d_modes.data_ptr()),
                     "sse": lambda: L.pnn_hevc_best_mode_device(ctx, w, d_p.data_ptr(), 2 * w + 1, 2 * w + 1, d_t.data_ptr(), n, index.data_ptr(),
                                                                sse.data_ptr(), None, None, sp)}
            if parent is not None:
                calls["parent"] = lambda: parent.pnn_trquant_device(parent_ctx, w, d_c.data_ptr(), d_t.data_ptr(), n, c_qps, nq,
                                                                    counts[0].data_ptr(), counts[1].data_ptr(), counts[2].data_ptr(), None, sp)
            # results first
            assert code(recon.data_ptr()) == 0
            torch.cuda.synchronize()
            m = min(n, 256)
            host = ip.transform_code(candidate[:m], targets[:m], QPS, keep_reconstructions=True)
            got = counts[:, :, :m].cpu().numpy().view(np.uint32)
            for k, name in enumerate(("sses_recon", "nb_nonzero_levels", "sum_abs_levels")):
                assert np.array_equal(got[k], host[name]), "w %d: %s differs from the host twin" % (w, name)
            assert np.array_equal(recon[:, :m].cpu().numpy(), host["reconstructions_uint8"]), "w %d: reconstructions differ from the host twin" % w
            mean_bits = {}
            for name, d_m, host_modes in (("tq_rate", None, None), ("tq_rate_modes", d_modes.data_ptr(), modes[:m])):
                assert code_rate(d_m) == 0
                torch.cuda.synchronize()
                host = ip.transform_code(candidate[:m], targets[:m], QPS, modes=host_modes, rate=True)
                assert np.array_equal(bits[:, :m].cpu().numpy().astype(np.float64) / 32768., host["rate_bits"]), "w %d: the rate differs from the host twin" % w
                got = counts[:, :, :m].cpu().numpy().view(np.uint32)
                for k, key in enumerate(("sses_recon", "nb_nonzero_levels", "sum_abs_levels")):
                    assert np.array_equal(got[k], host[key]), "w %d: %s differs from the host twin beside the rate" % (w, key)
                mean_bits[name] = float(bits.cpu().numpy().mean()) / 32768.
            plain_recon = recon[:, :m].cpu().numpy()
            for with_rate in (False, True):               # sign-data hiding: every output against the host twin
                assert code_sdh(bits.data_ptr() if with_rate else None, recon.data_ptr()) == 0
                torch.cuda.synchronize()
                host = ip.transform_code(candidate[:m], targets[:m], QPS, keep_reconstructions=True, rate=with_rate, sign_data_hiding=True)
                got = counts[:, :, :m].cpu().numpy().view(np.uint32)
                for k, key in enumerate(("sses_recon", "nb_nonzero_levels", "sum_abs_levels")):
                    assert np.array_equal(got[k], host[key]), "w %d: %s differs from the host twin under sign-data hiding" % (w, key)
                assert np.array_equal(recon[:, :m].cpu().numpy(), host["reconstructions_uint8"]), "w %d: hidden reconstructions differ" % w
                if with_rate:
                    assert np.array_equal(bits[:, :m].cpu().numpy().astype(np.float64) / 32768., host["rate_bits"]), "w %d: the hidden rate differs" % w
                    mean_bits["tq_rate_sdh"] = float(bits.cpu().numpy().mean()) / 32768.
            hidden_share = float((host["reconstructions_uint8"] != plain_recon).any(axis=(0, 2, 3)).mean())
            times = {name: [] for name in calls}
            for i in range(args.warmup + args.reps):
                order = list(calls)
                if parent is not None:                    # the two no-rate calls side by side, each first in turn: what runs in front of
                    order.remove("parent")                # a sample (and leaves its data in the caches) is then the same for both
                    order.remove("tq")
                    order = (["tq", "parent"] if i % 2 == 0 else ["parent", "tq"]) + order
                for name in order:
                    t = sample(torch, s, calls[name], args.calls)
                    if i >= args.warmup:
                        times[name].append(t)
            med = {name: statistics.median(v) for name, v in times.items()}
            fmt = lambda name: "%.1f [%.1f .. %.1f]" % (med[name], min(times[name]), max(times[name]))
            out("%-3d %8d %26s %12.4g %14.4g %26s %11.2fx" % (w, n, fmt("tq"), n / med["tq"] * 1e6, n * nq / med["tq"] * 1e6, fmt("sse"),
                                                               med["tq"] / med["sse"]))
            for name, label in (("tq_rate", "TQ+R"), ("tq_rate_modes", "TQ+R modes")):
                out("    %-12s %26s  %5.2fx TQ   (%.1f bits per block and QP on average)" % (label, fmt(name), med[name] / med["tq"], mean_bits[name]))
            out("    %-12s %26s  %5.2fx TQ   (hiding changed the reconstruction of %.0f %% of the blocks)"
                % ("TQ+H", fmt("tq_sdh"), med["tq_sdh"] / med["tq"], 100 * hidden_share))
            out("    %-12s %26s  %5.2fx TQ+R (%.1f bits per block and QP on average)"
                % ("TQ+R+H", fmt("tq_rate_sdh"), med["tq_rate_sdh"] / med["tq_rate"], mean_bits["tq_rate_sdh"]))
            if parent is not None:
                inside = min(times["parent"]) <= med["tq"] <= max(times["parent"])
                out("    %-12s %26s  TQ's median %.1f lies %s the parent's min .. max" % ("parent TQ", fmt("parent"), med["tq"], "INSIDE" if inside else "OUTSIDE"))


if __name__ == "__main__":
    main()
