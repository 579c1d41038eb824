"""What the scoring path from pictures buys, two comparisons on one box (writes profiles/picture_score_rate.txt):

  (a) end to end: evaluation.score_masks_from_pictures over a list of masks against a loop of
      evaluation.predict_mask_vs_hevc_best_mode over the same masks (the evaluator as it was: one upload, one descriptor loop,
      one context download, one host-array prediction, one Python PSNR loop and one dense-pattern upload per mask), same process,
      same nets, seeded pictures, w = 8 (the trained conv net) and w = 32 (seeded conv net).  Host clock around each whole call
      (both end in downloads, i.e. synchronised); the two alternate, the median of `--reps` runs after `--warmup` ones counts.
      Blocks/s = images x positions x masks / seconds.  The dictionaries are compared first: faster and different is not faster.
  (b) the search kernel: pnn_score_pictures_device asked for the HEVC index and SSE only (reference samples and targets read
      from the pictures, 4w + 1 + w^2 bytes per block) against pnn_hevc_best_mode_device on dense (2w + 1)^2 patterns and target
      copies of the same blocks, w = 8 and w = 64.  HIP events around each call, median of `--reps` alternating calls after
      `--warmup` ones.  The figure of the picture entry INCLUDES its read-back of the positions (the argument check), which the
      dense entry does not have: the comparison is conservative for the new path.

    python tools/picture_score_rate.py            # on the GPU box; --pairs adds the call on pairs of planes to (b)
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


def pictures(n_images, H, W, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for _ in range(n_images):
        f = rng.uniform(0.02, 0.2, 4)
        img = 128 + 60 * np.sin(f[0] * xx + f[1] * yy) + 40 * np.cos(f[2] * xx - f[3] * yy) + rng.normal(0, 6, (H, W))
        out.append(np.clip(img, 0, 255))
    return np.array(out).astype(np.uint8)


def end_to_end(args, out):
    import context_adaptive_neural_network_based_prediction_amd as P
    from context_adaptive_neural_network_based_prediction_amd import evaluation
    from tests import util
    out("# (a) end to end, %d warm-up + %d timed runs each, alternating; seconds per run over all masks (median [min .. max])" % (args.warmup, args.reps))
    out("%-3s %7s %-28s %22s %12s %22s %12s %8s" % ("w", "blocks", "masks", "old loop s", "blocks/s", "from pictures s", "blocks/s", "ratio"))
    for w, images, positions, masks in ((8, 4, 256, ((0, 0), (4, 4), (8, 8))), (32, 4, 64, ((0, 0), (16, 16), (32, 32)))):
        H, W = 512, 768
        imgs = pictures(images, H, W, 10 + w)[..., None]
        rng = np.random.default_rng(20 + w)
        rows = rng.integers(0, H - 3 * w + 1, positions).astype(np.int64)
        cols = rng.integers(0, W - 3 * w + 1, positions).astype(np.int64)
        n = images * positions
        if w == 8:
            net = P.PredictionNeuralNetwork(n, w, False, path_to_model=os.path.join(ROOT, "tests", "golden", "conv8_single.pnnw"))
        else:
            net = P.PredictionNeuralNetwork(n, w, False, params=util.make_params(w, False, seed=40 + w, out_gain=util.out_gain(w, False)))
        old = lambda: {m: evaluation.predict_mask_vs_hevc_best_mode(imgs, w, rows, cols, net, n, util.MEAN, m) for m in masks}
        new = lambda: evaluation.score_masks_from_pictures(imgs, w, rows, cols, net, util.MEAN, masks)
        a, b = old(), new()
        for m in masks:
            for key, v in a[m].items():
                same = v.tobytes() == b[m][key].tobytes() if isinstance(v, np.ndarray) else v == b[m][key]
                assert same, "w %d mask %s: '%s' differs between the two evaluators" % (w, m, key)
        times = {"old": [], "new": []}
        for i in range(args.warmup + args.reps):
            for name, fn in (("old", old), ("new", new)):
                t0 = time.perf_counter()
                fn()
                if i >= args.warmup:
                    times[name].append(time.perf_counter() - t0)
        med = {k: statistics.median(v) for k, v in times.items()}
        fmt = lambda k: "%.4f [%.4f .. %.4f]" % (med[k], min(times[k]), max(times[k]))
        total = n * len(masks)
        out("%-3d %7d %-28s %22s %12.4g %22s %12.4g %7.1fx" % (w, n, " ".join("(%d,%d)" % m for m in masks), fmt("old"), total / med["old"],
                                                              fmt("new"), total / med["new"], med["old"] / med["new"]))
        net.close()


def search_kernel(args, out):
    import torch

    from context_adaptive_neural_network_based_prediction_amd import _lib
    from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
    L = _lib.lib()
    ctx = ip._context(0)
    s = torch.cuda.current_stream()
    sp = ctypes.c_void_p(s.cuda_stream)
    out("# (b) best-mode search, index + SSE, %d warm-up + %d timed calls each, alternating; HIP events around each call, us per call (median [min .. max])"
        % (args.warmup, args.reps))
    out("%-3s %8s %12s %24s %12s %24s %12s %8s" % ("w", "blocks", "bytes/block", "dense patterns us", "blocks/s", "from pictures us", "blocks/s", "ratio"))
    for w, images, positions in ((8, 256, 4096), (64, 32, 1024)):
        H = W = 512
        imgs = pictures(4, H, W, 30 + w)
        imgs = np.concatenate([np.roll(imgs, 7 * k, axis=2) for k in range(images // 4)])
        rng = np.random.default_rng(40 + w)
        rows = rng.integers(0, H - 3 * w + 1, positions).astype(np.int64)
        cols = rng.integers(0, W - 3 * w + 1, positions).astype(np.int64)
        n = images * positions
        d_imgs = torch.from_numpy(imgs).cuda()
        d_rows, d_cols = torch.from_numpy(rows.astype(np.int32)).cuda(), torch.from_numpy(cols.astype(np.int32)).cuda()
        # the dense form of the same blocks, built on the device: first row and column of each (2w + 1)^2 pattern, the rest 255
        r = (d_rows.long() + w - 1)[:, None] + torch.arange(2 * w + 1, device="cuda")[None, :]
        c = (d_cols.long() + w - 1)[:, None] + torch.arange(2 * w + 1, device="cuda")[None, :]
        pats = torch.full((images, positions, 2 * w + 1, 2 * w + 1), 255, dtype=torch.uint8, device="cuda")
        pats[:, :, :, 0] = d_imgs[:, r, c[:, :1].expand(-1, 2 * w + 1)]
        pats[:, :, 0, :] = d_imgs[:, r[:, :1].expand(-1, 2 * w + 1), c]
        tr = (d_rows.long() + w)[:, None, None] + torch.arange(w, device="cuda")[None, :, None]
        tc = (d_cols.long() + w)[:, None, None] + torch.arange(w, device="cuda")[None, None, :]
        tgts = d_imgs[:, tr, tc].contiguous().view(n, w, w)
        pats = pats.view(n, 2 * w + 1, 2 * w + 1)
        res = {k: (torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")) for k in ("dense", "pic")}
        calls = {
            "dense": lambda: L.pnn_hevc_best_mode_device(ctx, w, pats.data_ptr(), 2 * w + 1, 2 * w + 1, tgts.data_ptr(), n, res["dense"][0].data_ptr(),
                                                         res["dense"][1].data_ptr(), None, None, sp),
            "pic": lambda: L.pnn_score_pictures_device(ctx, w, d_imgs.data_ptr(), images, H, W, d_rows.data_ptr(), d_cols.data_ptr(), positions, 0, 0,
                                                       None, None, None, None, res["pic"][0].data_ptr(), res["pic"][1].data_ptr(), None, sp)}
        if args.pairs:                                     # the same search on a pair: samples from an inverted copy, targets as before
            d_dec = 255 - d_imgs
            res["pair"] = (torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"))
            calls["pair"] = lambda: L.pnn_score_picture_pairs_device(ctx, w, d_dec.data_ptr(), d_imgs.data_ptr(), images, H, W, d_rows.data_ptr(),
                                                                     d_cols.data_ptr(), positions, 0, 0, None, None, None, None,
                                                                     res["pair"][0].data_ptr(), res["pair"][1].data_ptr(), None, sp)
        times = {name: [] for name in calls}
        for i in range(args.warmup + args.reps):
            for name in calls:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                assert calls[name]() == 0
                e1.record(s)
                e1.synchronize()
                if i >= args.warmup:
                    times[name].append(e0.elapsed_time(e1) * 1e3)
        assert torch.equal(res["dense"][0], res["pic"][0]) and torch.equal(res["dense"][1], res["pic"][1]), "w %d: the two searches differ" % w
        med = {k: statistics.median(v) for k, v in times.items()}
        fmt = lambda k: "%.1f [%.1f .. %.1f]" % (med[k], min(times[k]), max(times[k]))
        out("%-3d %8d %5d / %-5d %24s %12.4g %24s %12.4g %7.2fx" % (w, n, (2 * w + 1) ** 2 + w * w, 4 * w + 1 + w * w, fmt("dense"), n / med["dense"] * 1e6,
                                                                 fmt("pic"), n / med["pic"] * 1e6, med["dense"] / med["pic"]))
        if args.pairs:
            out("%-3d %8d   pair of planes, %d bytes/block: %s us, %.4g blocks/s, %.2fx the single-picture call"
                % (w, n, 4 * w + 1 + w * w, fmt("pair"), n / med["pair"] * 1e6, med["pic"] / med["pair"]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pairs", action="store_true", help="(b) also times pnn_score_picture_pairs_device (two planes) beside the single-picture call")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "picture_score_rate.txt"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        def out(line):
            print(line, flush=True)
            f.write(line + "\n")
        out("# tools/picture_score_rate.py on one %s; bytes/block = dense patterns + target copy / what the search from pictures reads" % torch.cuda.get_device_name(0))
        end_to_end(args, out)
        search_kernel(args, out)


if __name__ == "__main__":
    main()
