"""What HM's second intra pass costs as a column, on one box (appends to profiles/rd_pass.txt):

  pnn_rd_pass_device (the first-pass kernel, rd_candidates_kernel, the transform coding of the n (K + 1) candidate slots with the rate,
  rd_decide_kernel) on dense blocks, w = 8 with N = 65 536 and w = 32 with N = 8 192, at 4 QPs, beside the calls it extends: the
  first-pass call (FP: pnn_hevc_mode_hads_hm_device with a candidate) and the two transform calls with the rate (TQ PNN:
  pnn_trquant_sdh_device on the candidate, diagonal scan; TQ HEVC: on the same blocks with a mode array).  The entries alternate in one
  process; a sample is `--calls` back-to-back calls of one entry between two HIP events, the median and min .. max of `--reps` samples
  after `--warmup` ones count (the method of tools/trquant_rate.py).  Before anything is timed every output of pnn_rd_pass_device is
  compared with the host twin on the first blocks.  Reported: RD over FP + TQ PNN + TQ HEVC, and the split of RD between its
  launches, from samples of each launch's own entry on the shapes RD gives it (FP on n blocks; the transform call on n (K + 1) slots
  with the slots' modes; the rest of RD as the difference).  With --parent-lib, a libpnn_hip.so built from the parent commit joins
  the alternation for the three untouched calls: their medians here must lie inside the min .. max spread of the parent's samples.

    python tools/rd_pass_rate.py [--parent-lib /path/to/parent/libpnn_hip.so]          # on the GPU box
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
UNTOUCHED = ("fp", "tq_pnn", "tq_hevc")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10, help="back-to-back calls per timed sample")
    ap.add_argument("--parent-lib", default=None, help="libpnn_hip.so of the parent commit, for the untouched entries")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rd_pass.txt"))
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
        for name in ("pnn_create_empty", "pnn_hevc_mode_hads_hm_device", "pnn_trquant_sdh_device"):
            getattr(parent, name).restype, getattr(parent, name).argtypes = _lib.SIGNATURES[name]
        parent_ctx = ctypes.c_void_p()
        assert parent.pnn_create_empty(ctypes.byref(parent_ctx), ctypes.c_float(0.), 0) == 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        def out(line):
            print(line, flush=True)
            f.write(line + "\n")
        out("# tools/rd_pass_rate.py on one %s: %d warm-up + %d timed samples of %d back-to-back calls between two HIP events, entries"
            % (torch.cuda.get_device_name(0), args.warmup, args.reps, args.calls))
        out("# alternating; us per call, median [min .. max]; %d QPs %s; RD = pnn_rd_pass_device, FP = pnn_hevc_mode_hads_hm_device with a" % (nq, QPS))
        out("# candidate, TQ PNN / TQ HEVC = pnn_trquant_sdh_device with the rate (diagonal scan / a mode array), TQ slots = the same on RD's")
        out("# n (K + 1) slots with the slots' modes")
        for w, n in SHAPES:
            k = ip.first_pass_list_size(w)
            patterns, targets, candidate = blocks(w, n, 50 + w)
            d_p, d_t, d_c = (torch.from_numpy(a).cuda() for a in (patterns, targets, candidate))
            shapes = ip.rd_pass_shapes(n, nq, w)
            d_outs = [torch.zeros(int(np.prod(shape)) * np.dtype(dtype).itemsize, dtype=torch.uint8, device="cuda")
                      for (_, dtype), shape in zip(ip.RD_PASS_OUTPUTS, shapes)]
            nb_ws = L.pnn_rd_pass_workspace_bytes(w, n, nq)
            d_ws = torch.empty(nb_ws, dtype=torch.uint8, device="cuda")
            list_modes = torch.empty((n, k), dtype=torch.uint8, device="cuda")
            counts = torch.empty((nq, n * (k + 1)), dtype=torch.int32, device="cuda")
            bits = torch.empty((nq, n * (k + 1)), dtype=torch.int64, device="cuda")
            d_modes = torch.from_numpy((np.arange(n) % 35).astype(np.uint8)).cuda()
            slot_t, slot_c = d_t.repeat_interleave(k + 1, dim=0).contiguous(), d_c.repeat_interleave(k + 1, dim=0).contiguous()

            def rd():
                return L.pnn_rd_pass_device(ctx, w, d_p.data_ptr(), 2 * w + 1, 2 * w + 1, d_t.data_ptr(), n, d_c.data_ptr(), 0, c_qps, nq, None,
                                            0, *[o.data_ptr() for o in d_outs], d_ws.data_ptr(), nb_ws, sp)

            def fp(lib=L, c=ctx):
                return lib.pnn_hevc_mode_hads_hm_device(c, w, d_p.data_ptr(), 2 * w + 1, 2 * w + 1, d_t.data_ptr(), n, d_c.data_ptr(), 0, None,
                                                        None, list_modes.data_ptr(), None, sp)

            def tq(pred, tgt, count, modes, lib=L, c=ctx):
                return lib.pnn_trquant_sdh_device(c, w, pred.data_ptr(), tgt.data_ptr(), count, modes, c_qps, nq, counts.data_ptr(), None, None,
                                                  None, bits.data_ptr(), 0, sp)
            assert rd() == 0
            torch.cuda.synchronize()
            m = min(n, 256)
            host = ip.rd_pass(patterns[:m], targets[:m], candidate[:m], QPS)
            for (name, dtype), shape, d_o in zip(ip.RD_PASS_OUTPUTS, shapes, d_outs):
                got = d_o.cpu().numpy().view(dtype).reshape(shape)
                got = got[:m] if name == 'candidates' else got[:, :m]
                assert got.tobytes() == host[name].tobytes(), "w %d: %s differs from the host twin" % (w, name)
            slot_modes = d_outs[0]                        # the slots' modes RD left: the mode array of the transform call on the slots
            calls = {"rd": rd, "fp": fp, "tq_pnn": lambda: tq(d_c, d_t, n, None), "tq_hevc": lambda: tq(d_c, d_t, n, d_modes.data_ptr()),
                     "tq_slots": lambda: tq(slot_c, slot_t, n * (k + 1), slot_modes.data_ptr())}
            if parent is not None:
                calls.update({"parent_fp": lambda: fp(parent, parent_ctx), "parent_tq_pnn": lambda: tq(d_c, d_t, n, None, parent, parent_ctx),
                              "parent_tq_hevc": lambda: tq(d_c, d_t, n, d_modes.data_ptr(), parent, parent_ctx)})
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
            fmt = lambda name: "%.1f [%.1f .. %.1f]" % (med[name], min(times[name]), max(times[name]))
            extended = med["fp"] + med["tq_pnn"] + med["tq_hevc"]
            out("w %-3d N %-6d K + 1 = %d   RD %s   FP %s   TQ PNN %s   TQ HEVC %s" % (w, n, k + 1, fmt("rd"), fmt("fp"), fmt("tq_pnn"), fmt("tq_hevc")))
            out("    RD / (FP + TQ PNN + TQ HEVC) = %.2f   (%.4g blocks/s, %.4g candidate-QPs/s; PNN wins %.1f %% of the (QP, block) pairs)"
                % (med["rd"] / extended, n / med["rd"] * 1e6, n * (k + 1) * nq / med["rd"] * 1e6,
                   100 * float((d_outs[2].cpu().numpy() == 35).mean())))
            rest = med["rd"] - med["fp"] - med["tq_slots"]
            out("    split of RD: first pass %.0f %%, transform coding of the slots (TQ slots %s) %.0f %%, candidates + decision (the rest) %.0f %%"
                % (100 * med["fp"] / med["rd"], fmt("tq_slots"), 100 * med["tq_slots"] / med["rd"], 100 * rest / med["rd"]))
            for name in UNTOUCHED if parent is not None else ():
                inside = min(times["parent_" + name]) <= med[name] <= max(times["parent_" + name])
                out("    parent %-8s %26s  this build's median %.1f lies %s the parent's min .. max"
                    % (name, fmt("parent_" + name), med[name], "INSIDE" if inside else "OUTSIDE"))


if __name__ == "__main__":
    main()
