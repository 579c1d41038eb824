"""What HM's RDOQ costs in the transform-coding launch and in the second intra pass, on one box (appends to
profiles/rdoq.txt):

  pnn_trquant_rdoq_device with rdoq 1 beside rdoq 0 at 4 QPs, w = 8 with N = 65 536 and w = 32 with N = 8 192, with and without the
  rate (sign hiding on: the campaigns' setting), and pnn_rd_pass_rdoq_device with and without the option at the same shapes.  The
  entries alternate in one process; a sample is `--calls` back-to-back calls of one entry between two HIP events, the median and min ..
  max of `--reps` samples after `--warmup` ones count (the method of tools/trquant_rate.py).  Before anything is timed every output of
  the RDOQ calls is compared with the host twin on the first blocks.  Reported: the RDOQ / RDOQ-0 ratios and (RDOQ - RDOQ 0) / RDOQ,
  an UPPER ESTIMATE OF THE WHOLE RDOQ PATH, not of the walk alone: the difference also holds the fill of the bit estimates, the pass
  over the uncoded costs and two more barriers per QP, and it leaves out the plain quantiser (and signBitHidingHDQ) the path
  replaces.  No build with the walk stubbed out and no stamps were made.  With --parent-lib, a libpnn_hip.so built from the parent commit joins the alternation for the untouched calls (FP, TQ PNN,
  TQ HEVC, RD of section 5l's table): their medians here must lie inside the min .. max spread of the parent's samples.

    python tools/rdoq_rate.py [--parent-lib /path/to/parent/libpnn_hip.so]          # on the GPU box
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
UNTOUCHED = ("fp", "tq_pnn", "tq_hevc", "rd")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10, help="back-to-back calls per timed sample")
    ap.add_argument("--parent-lib", default=None, help="libpnn_hip.so of the parent commit, for the untouched entries")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rdoq.txt"))
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
        for name in ("pnn_create_empty", "pnn_hevc_mode_hads_hm_device", "pnn_trquant_sdh_device", "pnn_rd_pass_device"):
            getattr(parent, name).restype, getattr(parent, name).argtypes = _lib.SIGNATURES[name]
        parent_ctx = ctypes.c_void_p()
        assert parent.pnn_create_empty(ctypes.byref(parent_ctx), ctypes.c_float(0.), 0) == 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        def out(line):
            print(line, flush=True)
            f.write(line + "\n")
        out("# tools/rdoq_rate.py on one %s: %d warm-up + %d timed samples of %d back-to-back calls between two HIP events, entries"
            % (torch.cuda.get_device_name(0), args.warmup, args.reps, args.calls))
        out("# alternating; us per call, median [min .. max]; %d QPs %s, sign hiding on; TQ = pnn_trquant_rdoq_device with a mode array," % (nq, QPS))
        out("# RD = pnn_rd_pass_rdoq_device; `rdoq 1` / `rdoq 0` = the option on / off; no counter run was made: the bound of the new path is not known.")
        out("# `RDOQ path` = (rdoq 1 - rdoq 0) / rdoq 1: an upper estimate of the whole RDOQ path (bit estimates, uncoded costs, two barriers, the walk;")
        out("# less the plain quantiser it replaces), not of the walk alone: no build with the walk stubbed out, no stamps")
        for w, n in SHAPES:
            patterns, targets, candidate = blocks(w, n, 50 + w)
            d_p, d_t, d_c = (torch.from_numpy(a).cuda() for a in (patterns, targets, candidate))
            k = ip.first_pass_list_size(w)
            shapes = ip.rd_pass_shapes(n, nq, w)
            d_outs = [torch.zeros(int(np.prod(shape)) * np.dtype(dtype).itemsize, dtype=torch.uint8, device="cuda")
                      for (_, dtype), shape in zip(ip.RD_PASS_OUTPUTS, shapes)]
            nb_ws = L.pnn_rd_pass_workspace_bytes(w, n, nq)
            d_ws = torch.empty(nb_ws, dtype=torch.uint8, device="cuda")
            list_modes = torch.empty((n, k), dtype=torch.uint8, device="cuda")
            counts = torch.zeros((3, nq, n), dtype=torch.int32, device="cuda")
            bits = torch.zeros((nq, n), dtype=torch.int64, device="cuda")
            modes = (np.arange(n) % 35).astype(np.uint8)
            d_modes = torch.from_numpy(modes).cuda()

            def tq(rdoq, rate, flag=1):
                return L.pnn_trquant_rdoq_device(ctx, w, d_c.data_ptr(), d_t.data_ptr(), n, d_modes.data_ptr(), c_qps, nq, counts[0].data_ptr(),
                                                 counts[1].data_ptr(), counts[2].data_ptr(), None, bits.data_ptr() if rate else None, flag, rdoq,
                                                 None, sp)

            def rd(rdoq):
                return L.pnn_rd_pass_rdoq_device(ctx, w, d_p.data_ptr(), 2 * w + 1, 2 * w + 1, d_t.data_ptr(), n, d_c.data_ptr(), 0, c_qps, nq, None,
                                                 1, rdoq, *[o.data_ptr() for o in d_outs], d_ws.data_ptr(), nb_ws, sp)

            def old_fp(lib=L, c=ctx):
                return lib.pnn_hevc_mode_hads_hm_device(c, w, d_p.data_ptr(), 2 * w + 1, 2 * w + 1, d_t.data_ptr(), n, d_c.data_ptr(), 0, None,
                                                        None, list_modes.data_ptr(), None, sp)

            def old_tq(mode_ptr, lib=L, c=ctx):
                return lib.pnn_trquant_sdh_device(c, w, d_c.data_ptr(), d_t.data_ptr(), n, mode_ptr, c_qps, nq, counts[0].data_ptr(), None, None,
                                                  None, bits.data_ptr(), 0, sp)

            def old_rd(lib=L, c=ctx):
                return lib.pnn_rd_pass_device(c, w, d_p.data_ptr(), 2 * w + 1, 2 * w + 1, d_t.data_ptr(), n, d_c.data_ptr(), 0, c_qps, nq, None,
                                              0, *[o.data_ptr() for o in d_outs], d_ws.data_ptr(), nb_ws, sp)
            # every output against the host twin first, on the first blocks
            m = min(n, 256)
            assert tq(1, True) == 0
            torch.cuda.synchronize()
            host = ip.transform_code(candidate[:m], targets[:m], QPS, modes=modes[:m], rate=True, sign_data_hiding=True, rdoq=True)
            got = counts.cpu().numpy().view(np.uint32)
            for i, name in enumerate(('sses_recon', 'nb_nonzero_levels', 'sum_abs_levels')):
                assert np.array_equal(got[i][:, :m], host[name]), "w %d: %s differs from the host twin" % (w, name)
            assert np.array_equal(bits.cpu().numpy()[:, :m].astype(np.float64) / 32768., host['rate_bits']), "w %d: the rate differs" % w
            assert rd(1) == 0
            torch.cuda.synchronize()
            host = ip.rd_pass(patterns[:m], targets[:m], candidate[:m], QPS, sign_data_hiding=True, rdoq=True)
            for (name, dtype), shape, d_o in zip(ip.RD_PASS_OUTPUTS, shapes, d_outs):
                got = d_o.cpu().numpy().view(dtype).reshape(shape)
                got = got[:m] if name == 'candidates' else got[:, :m]
                assert got.tobytes() == host[name].tobytes(), "w %d: %s differs from the host twin" % (w, name)
            calls = {"tq1_rate": lambda: tq(1, True), "tq0_rate": lambda: tq(0, True), "tq1": lambda: tq(1, False), "tq0": lambda: tq(0, False),
                     "rd1": lambda: rd(1), "rd0": lambda: rd(0), "fp": old_fp, "tq_pnn": lambda: old_tq(None),
                     "tq_hevc": lambda: old_tq(d_modes.data_ptr()), "rd": old_rd}
            if parent is not None:
                calls.update({"parent_fp": lambda: old_fp(parent, parent_ctx), "parent_tq_pnn": lambda: old_tq(None, parent, parent_ctx),
                              "parent_tq_hevc": lambda: old_tq(d_modes.data_ptr(), parent, parent_ctx), "parent_rd": lambda: old_rd(parent, parent_ctx)})
            times = {name: [] for name in calls}
            for i in range(args.warmup + args.reps):
                order = list(calls)
                if i % 2:                                 # each entry in front of and behind its neighbours in turn
                    order.reverse()
                for name in order:
                    t = sample(torch, s, calls[name], args.calls)
                    if i >= args.warmup:
                        times[name].append(t)
            med = {name: statistics.median(v) for name, v in times.items()}
            fmt = lambda name: "%.1f [%.1f .. %.1f]" % (med[name], min(times[name]), max(times[name]))  # noqa: E731
            out("w %-3d N %-6d" % (w, n))
            for one, zero, label in (("tq1_rate", "tq0_rate", "TQ with the rate"), ("tq1", "tq0", "TQ without the rate"), ("rd1", "rd0", "RD")):
                out("    %-20s rdoq 1 %s   rdoq 0 %s   ratio %.2f   RDOQ path %.0f %%"
                    % (label, fmt(one), fmt(zero), med[one] / med[zero], 100 * (med[one] - med[zero]) / med[one]))
            for name in UNTOUCHED if parent is not None else ():
                inside = min(times["parent_" + name]) <= med[name] <= max(times["parent_" + name])
                out("    parent %-8s %30s  this build's median %.1f lies %s the parent's min .. max"
                    % (name, fmt("parent_" + name), med[name], "INSIDE" if inside else "OUTSIDE"))


if __name__ == "__main__":
    main()
