"""What the first-pass ranking costs beside the SSE search it is the twin of, on one box (writes profiles/hevc_mode_hads_rate.txt):

  hevc_mode_hads_kernel (pnn_hevc_mode_hads_device: per-mode Hadamard costs, the candidate's cost and the sorted list) against
  hevc_best_mode_kernel (pnn_hevc_best_mode_device: index + SSE) on the SAME dense blocks, w = 8 with N = 65 536 and w = 32 with
  N = 8 192 (the shapes of profiles/hevc_best_mode_rate.txt).  The two alternate in one process; a sample is `--calls` back-to-back
  calls of one entry between two HIP events (one call is 0.1 ms: too short a window on its own), the median of `--reps` samples
  after `--warmup` ones counts.  Before anything is timed the SATD outputs are compared with the host twin on the first blocks and
  the SSE search with its own per-mode output: faster and different is not faster.
  "x SSE search" is the figure to read: the SATD kernel does the search's prediction work per pixel (through the general per-pixel
  form, not the row walk) plus about 2 T^2 log2 T additions per T x T sub-block, and writes 35 + 1 + 2K values per block, not 2.

    python tools/hevc_mode_hads_rate.py           # on the GPU box

  --smoothing (writes profiles/hevc_smoothing_rate.txt): what HM's reference-sample smoothing costs in both kernels.  The *_hm entries
  with smoothing = 0 (the instantiations the older entries launch) and smoothing = 2 (the SMOOTH instantiations: one more LDS pass over
  4w + 1 samples per block, a second line in LDS) alternate in one process on the same dense blocks, same method, after both have been
  compared with the host twin; the present sizes plus w = 16 with N = 32 768.  The smoothing = 0 column is the yardstick of the
  smoothing = 2 one; the brackets of profiles/hevc_mode_hads_rate.txt (the parent's kernels, another run) are printed beside it.

    python tools/hevc_mode_hads_rate.py --smoothing
"""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((8, 65536), (32, 8192))
SMOOTHING_SHAPES = ((8, 65536), (16, 32768), (32, 8192))


def blocks(w, n, seed):
    """Seeded dense blocks with structure: patterns [n, 2w+1, 2w+1] (first row and column from a smooth picture plus noise, the
    rest 255), targets [n, w, w], a candidate near the target."""
    rng = np.random.default_rng(seed)
    n_all, n = n, min(n, 1024)                      # 1024 distinct blocks, repeated: the kernels' time does not depend on the values
    side = 3 * w
    yy, xx = np.mgrid[0:side, 0:side]
    f = rng.uniform(0.02, 0.3, (n, 4, 1, 1))
    img = 128 + 60 * np.sin(f[:, 0] * xx + f[:, 1] * yy) + 40 * np.cos(f[:, 2] * xx - f[:, 3] * yy) + rng.normal(0, 6, (n, side, side))
    img = np.clip(img, 0, 255).astype(np.uint8)
    patterns = np.full((n, 2 * w + 1, 2 * w + 1), 255, np.uint8)
    patterns[:, 0, :] = img[:, w - 1, w - 1:]
    patterns[:, :, 0] = img[:, w - 1:, w - 1]
    targets = np.ascontiguousarray(img[:, w:2 * w, w:2 * w])
    candidate = np.clip(targets.astype(np.int64) + rng.integers(-8, 9, targets.shape), 0, 255).astype(np.uint8)
    return tuple(np.ascontiguousarray(np.tile(a, (n_all // n, 1, 1))) for a in (patterns, targets, candidate))


def sample(torch, s, call, nb_calls):
    """us per call of `nb_calls` back-to-back calls between two HIP events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(nb_calls):
        assert call() == 0
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / nb_calls


def parent_brackets(path):
    """{w: (SATD bracket, SSE bracket)} as profiles/hevc_mode_hads_rate.txt holds them: the figures of the kernels before the SMOOTH axis"""
    brackets = {}
    if os.path.exists(path):
        for line in open(path):
            if not line.startswith(("#", "w")) and line.count("[") == 2:
                parts = line.replace("[", " [").split()
                both = [b.split("]")[0] for b in line.split("[")[1:]]
                brackets[int(parts[0])] = ("[" + both[0] + "]", "[" + both[1] + "]")
    return brackets


def smoothing_rate(args):
    import torch
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    from context_adaptive_neural_network_based_prediction_amd import _lib
    from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
    L = _lib.lib()
    ctx = ip._context(0)
    s = torch.cuda.current_stream()
    sp = ctypes.c_void_p(s.cuda_stream)
    path = args.out or os.path.join(ROOT, "profiles", "hevc_smoothing_rate.txt")
    parent = parent_brackets(os.path.join(ROOT, "profiles", "hevc_mode_hads_rate.txt"))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        def out(line):
            print(line, flush=True)
            f.write(line + "\n")
        out("# tools/hevc_mode_hads_rate.py --smoothing on one %s: %d warm-up + %d timed samples each, alternating; a sample = %d back-to-back calls"
            % (torch.cuda.get_device_name(0), args.warmup, args.reps, args.calls))
        out("# between two HIP events; us per call (median [min .. max]); SATD = pnn_hevc_mode_hads_hm_device (costs + candidate + list), SSE =")
        out("# pnn_hevc_best_mode_hm_device (index + SSE); s0 = smoothing 0 (the older entries' kernels), s2 = smoothing 2 (HM: [1 2 1] and strong);")
        out("# parent = the [min .. max] of profiles/hevc_mode_hads_rate.txt (the kernels before this option, an earlier run), where it has the size")
        out("%-3s %6s %-5s %26s %26s %8s %20s" % ("w", "N", "", "s0 us/call", "s2 us/call", "s2 / s0", "parent"))
        for w, n in SMOOTHING_SHAPES:
            patterns, targets, candidate = blocks(w, n, 50 + w)
            k = ip.first_pass_list_size(w)
            d_p, d_t, d_c = (torch.from_numpy(a).cuda() for a in (patterns, targets, candidate))
            hads = torch.empty((n, 35), dtype=torch.int32, device="cuda")
            cand = torch.empty(n, dtype=torch.int32, device="cuda")
            modes = torch.empty((n, k), dtype=torch.uint8, device="cuda")
            costs = torch.empty((n, k), dtype=torch.int32, device="cuda")
            index = torch.empty(n, dtype=torch.uint8, device="cuda")
            sse = torch.empty(n, dtype=torch.int32, device="cuda")
            all_sse = torch.empty((n, 35), dtype=torch.int32, device="cuda")
            side = 2 * w + 1

            def satd(smoothing):
                return L.pnn_hevc_mode_hads_hm_device(ctx, w, d_p.data_ptr(), side, side, d_t.data_ptr(), n, d_c.data_ptr(), smoothing, hads.data_ptr(),
                                                      cand.data_ptr(), modes.data_ptr(), costs.data_ptr(), sp)

            def search(smoothing, per_mode=None):
                return L.pnn_hevc_best_mode_hm_device(ctx, w, d_p.data_ptr(), side, side, d_t.data_ptr(), n, smoothing, index.data_ptr(), sse.data_ptr(),
                                                      None, per_mode, sp)
            # results first: both kernels, both settings, against the host twin on the first blocks
            m = min(n, 256)
            for smoothing in (0, 2):
                assert satd(smoothing) == 0 and search(smoothing, all_sse.data_ptr()) == 0
                torch.cuda.synchronize()
                host = ip.mode_hads_host(patterns[:m], targets[:m], w, candidate[:m], smoothing=smoothing)
                assert np.array_equal(hads[:m].cpu().numpy().view(np.uint32), host["hads_modes"]), "w %d: per-mode costs differ from the host twin" % w
                assert np.array_equal(cand[:m].cpu().numpy().view(np.uint32), host["hads_candidate"])
                assert np.array_equal(modes[:m].cpu().numpy(), host["list_modes"]) and np.array_equal(costs[:m].cpu().numpy().view(np.uint32), host["list_costs"])
                preds = np.array([[ip.predict_via_hevc_mode(np.ascontiguousarray(p[..., None]), w, mode, smoothing=smoothing)[..., 0] for mode in range(35)]
                                  for p in patterns[:32]], np.int64)
                want = ((preds - targets[:32, None].astype(np.int64)) ** 2).sum(axis=(2, 3))
                assert np.array_equal(all_sse[:32].cpu().numpy().view(np.uint32), want), "w %d: per-mode SSEs differ from the host twin" % w
                assert torch.equal(all_sse.min(dim=1).values, sse)
            calls = {("satd", 0): lambda: satd(0), ("satd", 2): lambda: satd(2), ("sse", 0): lambda: search(0), ("sse", 2): lambda: search(2)}
            times = {name: [] for name in calls}
            for i in range(args.warmup + args.reps):
                for name in calls:
                    t = sample(torch, s, calls[name], args.calls)
                    if i >= args.warmup:
                        times[name].append(t)
            med = {name: statistics.median(v) for name, v in times.items()}
            fmt = lambda name: "%.1f [%.1f .. %.1f]" % (med[name], min(times[name]), max(times[name]))
            for j, kernel in enumerate(("satd", "sse")):
                out("%-3d %6d %-5s %26s %26s %7.3fx %20s" % (w, n, kernel.upper(), fmt((kernel, 0)), fmt((kernel, 2)), med[(kernel, 2)] / med[(kernel, 0)],
                                                            parent[w][j] if w in parent else "-"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20, help="back-to-back calls per timed sample")
    ap.add_argument("--out", default=None, help="default: profiles/hevc_mode_hads_rate.txt, with --smoothing profiles/hevc_smoothing_rate.txt")
    ap.add_argument("--smoothing", action="store_true", help="time smoothing = 0 against smoothing = 2 in both kernels instead")
    args = ap.parse_args()
    if args.smoothing:
        return smoothing_rate(args)
    args.out = args.out or os.path.join(ROOT, "profiles", "hevc_mode_hads_rate.txt")
    import torch
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    from context_adaptive_neural_network_based_prediction_amd import _lib
    from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
    L = _lib.lib()
    ctx = ip._context(0)
    s = torch.cuda.current_stream()
    sp = ctypes.c_void_p(s.cuda_stream)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        def out(line):
            print(line, flush=True)
            f.write(line + "\n")
        out("# tools/hevc_mode_hads_rate.py on one %s: %d warm-up + %d timed samples each, alternating; a sample = %d back-to-back calls between"
            % (torch.cuda.get_device_name(0), args.warmup, args.reps, args.calls))
        out("# two HIP events; us per call (median [min .. max]); SATD = pnn_hevc_mode_hads_device (costs + candidate + list), SSE = pnn_hevc_best_mode_device (index + SSE)")
        out("%-3s %8s %26s %12s %26s %12s %12s" % ("w", "N", "SATD us/call", "blocks/s", "SSE us/call", "blocks/s", "x SSE search"))
        for w, n in SHAPES:
            patterns, targets, candidate = blocks(w, n, 50 + w)
            k = ip.first_pass_list_size(w)
            d_p, d_t, d_c = (torch.from_numpy(a).cuda() for a in (patterns, targets, candidate))
            hads = torch.empty((n, 35), dtype=torch.int32, device="cuda")
            cand = torch.empty(n, dtype=torch.int32, device="cuda")
            modes = torch.empty((n, k), dtype=torch.uint8, device="cuda")
            costs = torch.empty((n, k), dtype=torch.int32, device="cuda")
            index = torch.empty(n, dtype=torch.uint8, device="cuda")
            sse = torch.empty(n, dtype=torch.int32, device="cuda")
            all_sse = torch.empty((n, 35), dtype=torch.int32, device="cuda")
            calls = {
                "satd": lambda: L.pnn_hevc_mode_hads_device(ctx, w, d_p.data_ptr(), 2 * w + 1, 2 * w + 1, d_t.data_ptr(), n, d_c.data_ptr(), hads.data_ptr(),
                                                            cand.data_ptr(), modes.data_ptr(), costs.data_ptr(), sp),
                "sse": lambda: L.pnn_hevc_best_mode_device(ctx, w, d_p.data_ptr(), 2 * w + 1, 2 * w + 1, d_t.data_ptr(), n, index.data_ptr(), sse.data_ptr(),
                                                           None, None, sp)}
            # results first
            assert calls["satd"]() == 0
            assert L.pnn_hevc_best_mode_device(ctx, w, d_p.data_ptr(), 2 * w + 1, 2 * w + 1, d_t.data_ptr(), n, index.data_ptr(), sse.data_ptr(), None,
                                               all_sse.data_ptr(), sp) == 0
            torch.cuda.synchronize()
            m = min(n, 256)
            host = ip.mode_hads_host(patterns[:m], targets[:m], w, candidate[:m])
            assert np.array_equal(hads[:m].cpu().numpy().view(np.uint32), host["hads_modes"]), "w %d: per-mode costs differ from the host twin" % w
            assert np.array_equal(cand[:m].cpu().numpy().view(np.uint32), host["hads_candidate"]), "w %d: candidate costs differ from the host twin" % w
            assert np.array_equal(modes[:m].cpu().numpy(), host["list_modes"]) and np.array_equal(costs[:m].cpu().numpy().view(np.uint32), host["list_costs"])
            assert torch.equal(all_sse.min(dim=1).values, sse), "w %d: the SSE search differs from its own per-mode output" % w
            times = {name: [] for name in calls}
            for i in range(args.warmup + args.reps):
                for name in calls:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    for _ in range(args.calls):
                        assert calls[name]() == 0
                    e1.record(s)
                    e1.synchronize()
                    if i >= args.warmup:
                        times[name].append(e0.elapsed_time(e1) * 1e3 / args.calls)
            med = {name: statistics.median(v) for name, v in times.items()}
            fmt = lambda name: "%.1f [%.1f .. %.1f]" % (med[name], min(times[name]), max(times[name]))
            out("%-3d %8d %26s %12.4g %26s %12.4g %11.2fx" % (w, n, fmt("satd"), n / med["satd"] * 1e6, fmt("sse"), n / med["sse"] * 1e6,
                                                             med["satd"] / med["sse"]))


if __name__ == "__main__":
    main()
