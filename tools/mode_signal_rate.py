"""What the second pass costs with mode signalling, on one box (appends to profiles/mode_signal.txt):

  pnn_rd_pass_signal_device with signalling 1 (SG: the first-pass kernel, signal_list_kernel, then per QP the slots form of
  rd_candidates_kernel, the transform coding of the n (K + 3) slots at that QP and rd_decide_signal_kernel) beside
  pnn_rd_pass_rdoq_device (RD) on the same dense blocks, w = 8 with N = 65 536 and w = 32 with N = 8 192, 4 QPs, RDOQ off, seeded
  neighbour modes.  The entries alternate in one process; a sample is `--calls` back-to-back calls of one entry between two HIP events,
  the median and min .. max of `--reps` samples after `--warmup` ones count (the method of tools/rd_pass_rate.py).  Before anything is
  timed every output of SG is compared with the host twin on the first blocks.  Reported: SG / RD beside (K + 3) / (K + 1), and the
  split of SG from samples of its launches' own entries on the shapes SG gives them: HADS (the first-pass call asked for the costs, no
  list), TQ slots (nb_qps calls of the transform entry, one QP each, on the n (K + 3) slots with the slots' modes) and the rest --
  signal_list_kernel, the candidates and the decisions together, a difference, not timed alone.  With --parent-lib, a libpnn_hip.so
  built from the parent commit joins the alternation for the calls whose kernels and launches are the parent's (FP, TQ PNN, TQ HEVC, RD
  and SG itself): their medians here must lie inside the min .. max spread of the parent's samples.

    python tools/mode_signal_rate.py [--parent-lib /path/to/parent/libpnn_hip.so]          # on the GPU box
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
UNTOUCHED = ("fp", "tq_pnn", "tq_hevc", "rd", "sg")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10, help="back-to-back calls per timed sample")
    ap.add_argument("--parent-lib", default=None, help="libpnn_hip.so of the parent commit, for the untouched entries")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mode_signal.txt"))
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
    one_qp = [(ctypes.c_int * 1)(q) for q in QPS]
    parent = parent_ctx = None
    if args.parent_lib:
        parent = ctypes.CDLL(args.parent_lib)
        for name in ("pnn_create_empty", "pnn_hevc_mode_hads_hm_device", "pnn_trquant_sdh_device", "pnn_rd_pass_rdoq_device",
                     "pnn_rd_pass_signal_device"):
            getattr(parent, name).restype, getattr(parent, name).argtypes = _lib.SIGNATURES[name]
        parent_ctx = ctypes.c_void_p()
        assert parent.pnn_create_empty(ctypes.byref(parent_ctx), ctypes.c_float(0.), 0) == 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        def out(line):
            print(line, flush=True)
            f.write(line + "\n")
        out("# tools/mode_signal_rate.py on one %s: %d warm-up + %d timed samples of %d back-to-back calls between two HIP events, entries"
            % (torch.cuda.get_device_name(0), args.warmup, args.reps, args.calls))
        out("# alternating; us per call, median [min .. max]; %d QPs %s, RDOQ off; SG = pnn_rd_pass_signal_device (signalling 1, seeded" % (nq, QPS))
        out("# neighbours), RD = pnn_rd_pass_rdoq_device, HADS = pnn_hevc_mode_hads_hm_device asked for the costs, TQ slots = %d calls of" % nq)
        out("# pnn_trquant_rdoq_device, one QP each, on SG's n (K + 3) slots; FP, TQ PNN, TQ HEVC as in tools/rd_pass_rate.py")
        for w, n in SHAPES:
            k = ip.first_pass_list_size(w)
            slots = ip.rd_pass_slot_count(w, True)
            patterns, targets, candidate = blocks(w, n, 50 + w)
            rng = np.random.default_rng(90 + w)
            left, above = (np.where(rng.random(n) < 0.2, 255, rng.integers(0, 36, n)).astype(np.uint8) for _ in range(2))
            d_p, d_t, d_c, d_l, d_a = (torch.from_numpy(a).cuda() for a in (patterns, targets, candidate, left, above))
            sg_shapes, rd_shapes = ip.rd_pass_signal_shapes(n, nq, w), ip.rd_pass_shapes(n, nq, w)
            make = lambda outputs, shapes: [torch.zeros(int(np.prod(shape)) * np.dtype(dtype).itemsize, dtype=torch.uint8, device="cuda")
                                            for (_, dtype), shape in zip(outputs, shapes)]
            sg_outs, rd_outs = make(ip.RD_PASS_SIGNAL_OUTPUTS, sg_shapes), make(ip.RD_PASS_OUTPUTS, rd_shapes)
            nb_sg, nb_rd = L.pnn_rd_pass_signal_workspace_bytes(w, n, nq, 1), L.pnn_rd_pass_workspace_bytes(w, n, nq)
            d_ws = torch.empty(max(nb_sg, nb_rd), dtype=torch.uint8, device="cuda")
            hads, cand_hads = torch.empty((n, 35), dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
            list_modes = torch.empty((n, k), dtype=torch.uint8, device="cuda")
            counts = torch.empty((nq, n * slots), dtype=torch.int32, device="cuda")
            bits = torch.empty((nq, n * slots), dtype=torch.int64, device="cuda")
            d_modes = torch.from_numpy((np.arange(n) % 35).astype(np.uint8)).cuda()
            slot_t, slot_c = d_t.repeat_interleave(slots, dim=0).contiguous(), d_c.repeat_interleave(slots, dim=0).contiguous()
            blocks_args = (w, d_p.data_ptr(), 2 * w + 1, 2 * w + 1, d_t.data_ptr(), n, d_c.data_ptr(), 0)

            def sg(lib=L, c=ctx):
                return lib.pnn_rd_pass_signal_device(c, *blocks_args, c_qps, nq, None, 0, 0, 1, d_l.data_ptr(), d_a.data_ptr(),
                                                     *[o.data_ptr() for o in sg_outs], d_ws.data_ptr(), nb_sg, sp)

            def rd(lib=L, c=ctx):
                return lib.pnn_rd_pass_rdoq_device(c, *blocks_args, c_qps, nq, None, 0, 0, *[o.data_ptr() for o in rd_outs], d_ws.data_ptr(), nb_rd, sp)

            def fp(lib=L, c=ctx):
                return lib.pnn_hevc_mode_hads_hm_device(c, *blocks_args, None, None, list_modes.data_ptr(), None, sp)

            def hads_call():
                return L.pnn_hevc_mode_hads_hm_device(ctx, *blocks_args, hads.data_ptr(), cand_hads.data_ptr(), None, None, sp)

            def tq(pred, tgt, count, modes, lib=L, c=ctx):
                return lib.pnn_trquant_sdh_device(c, w, pred.data_ptr(), tgt.data_ptr(), count, modes, c_qps, nq, counts.data_ptr(), None, None,
                                                  None, bits.data_ptr(), 0, sp)

            def tq_slots():
                rc = 0
                for qi in range(nq):                      # what SG launches: one QP per call, with the count of nonzero levels
                    rc |= L.pnn_trquant_rdoq_device(ctx, w, slot_c.data_ptr(), slot_t.data_ptr(), n * slots, sg_outs[0].data_ptr(), one_qp[qi], 1,
                                                    counts.data_ptr(), counts[1].data_ptr(), None, None, bits.data_ptr(), 0, 0, None, sp)
                return rc
            assert sg() == 0
            torch.cuda.synchronize()
            m = min(n, 256)
            host = ip.rd_pass(patterns[:m], targets[:m], candidate[:m], QPS, signalling=True, neighbour_modes=(left[:m], above[:m]))
            for (name, dtype), shape, d_o in zip(ip.RD_PASS_SIGNAL_OUTPUTS, sg_shapes, sg_outs):
                got = d_o.cpu().numpy().view(dtype).reshape(shape)[:, :m]
                assert got.tobytes() == host[name].tobytes(), "w %d: %s differs from the host twin" % (w, name)
            pnn_wins = 100 * float((sg_outs[2].cpu().numpy() == 35).mean())
            assert rd() == 0
            torch.cuda.synchronize()
            pnn_wins_rd = 100 * float((rd_outs[2].cpu().numpy() == 35).mean())
            calls = {"sg": sg, "rd": rd, "fp": fp, "hads": hads_call, "tq_pnn": lambda: tq(d_c, d_t, n, None),
                     "tq_hevc": lambda: tq(d_c, d_t, n, d_modes.data_ptr()), "tq_slots": tq_slots}
            if parent is not None:
                calls.update({"parent_fp": lambda: fp(parent, parent_ctx), "parent_tq_pnn": lambda: tq(d_c, d_t, n, None, parent, parent_ctx),
                              "parent_tq_hevc": lambda: tq(d_c, d_t, n, d_modes.data_ptr(), parent, parent_ctx),
                              "parent_rd": lambda: rd(parent, parent_ctx), "parent_sg": lambda: sg(parent, parent_ctx)})
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
            out("w %-3d N %-6d K + 3 = %d   SG %s   RD %s   SG / RD = %.2f   ((K + 3) / (K + 1) = %.2f)"
                % (w, n, slots, fmt("sg"), fmt("rd"), med["sg"] / med["rd"], slots / (k + 1.)))
            out("    PNN wins %.1f %% of the (QP, block) pairs with signalling, %.1f %% without" % (pnn_wins, pnn_wins_rd))
            rest = med["sg"] - med["hads"] - med["tq_slots"]
            out("    split of SG: Hadamard costs (HADS %s) %.0f %%, coding of the slots (TQ slots %s) %.0f %%, list kernel + candidates + decisions (the rest) %.0f %%"
                % (fmt("hads"), 100 * med["hads"] / med["sg"], fmt("tq_slots"), 100 * med["tq_slots"] / med["sg"], 100 * rest / med["sg"]))
            out("    FP %s   TQ PNN %s   TQ HEVC %s" % (fmt("fp"), fmt("tq_pnn"), fmt("tq_hevc")))
            for name in UNTOUCHED if parent is not None else ():
                inside = min(times["parent_" + name]) <= med[name] <= max(times["parent_" + name])
                out("    parent %-8s %26s  this build's median %.1f lies %s the parent's min .. max"
                    % (name, fmt("parent_" + name), med[name], "INSIDE" if inside else "OUTSIDE"))

        # the second pass at w = 64: the two instantiations of rd_candidates_kernel<64> it launches are the only existing kernels whose
        # assembly is not the parent's line for line, so the entry is timed against the parent's library too
        w, n = 64, 2048
        patterns, targets, candidate = blocks(w, n, 50 + w)
        d_p, d_t, d_c = (torch.from_numpy(a).cuda() for a in (patterns, targets, candidate))
        rd_outs = [torch.zeros(int(np.prod(shape)) * np.dtype(dtype).itemsize, dtype=torch.uint8, device="cuda")
                   for (_, dtype), shape in zip(ip.RD_PASS_OUTPUTS, ip.rd_pass_shapes(n, nq, w))]
        nb_rd = L.pnn_rd_pass_workspace_bytes(w, n, nq)
        d_ws = torch.empty(nb_rd, dtype=torch.uint8, device="cuda")

        def rd64(lib=L, c=ctx):
            return lib.pnn_rd_pass_rdoq_device(c, w, d_p.data_ptr(), 2 * w + 1, 2 * w + 1, d_t.data_ptr(), n, d_c.data_ptr(), 0, c_qps, nq, None, 0, 0,
                                               *[o.data_ptr() for o in rd_outs], d_ws.data_ptr(), nb_rd, sp)
        calls = {"rd": rd64}
        if parent is not None:
            calls["parent_rd"] = lambda: rd64(parent, parent_ctx)
        times = {name: [] for name in calls}
        for i in range(args.warmup + args.reps):
            for name in (list(calls)[::-1] if i % 2 else list(calls)):
                assert calls[name]() == 0
                t = sample(torch, s, calls[name], args.calls)
                if i >= args.warmup:
                    times[name].append(t)
        med = {name: statistics.median(v) for name, v in times.items()}
        out("w 64  N %d   RD %.1f [%.1f .. %.1f]" % (n, med["rd"], min(times["rd"]), max(times["rd"])))
        if parent is not None:
            inside = min(times["parent_rd"]) <= med["rd"] <= max(times["parent_rd"])
            out("    parent rd %.1f [%.1f .. %.1f]  this build's median %.1f lies %s the parent's min .. max"
                % (med["parent_rd"], min(times["parent_rd"]), max(times["parent_rd"]), med["rd"], "INSIDE" if inside else "OUTSIDE"))


if __name__ == "__main__":
    main()
