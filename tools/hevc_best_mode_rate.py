"""Rate of the HEVC best-intra-mode search (the evaluator's competitor), three ways:

  --gpu   pnn_hevc_best_mode_device per width at N where the launch cost is negligible (and at N / 8 beside it): kernel time
          from HIP events around `--reps` back-to-back calls after `--warmup` ones, blocks/s, pixel-mode evaluations/s
          (35 w^2 per block) and what the integer VALU roof allows per evaluation.  The roof is the spec sheet's
          256 CU x 4 SIMD x 32 lanes x 2.4 GHz = 78.6 T lane-ops/s, not a measurement.
  --host  the host twin pnn_hevc_intra_predict over `--threads` OpenMP threads (tools/hevc_host_rate.cpp, built here with g++
          into tools/_bin/): 35 calls + SSE + argmin per block, random full patterns.
  --ref   the reference's own Python / Cython loop (intraprediction.predict_series_via_hevc_best_mode) on a small sample;
          needs the reference checkout (tests/golden/make_hevc_intra_golden.py builds it in a temporary directory).

    python tools/hevc_best_mode_rate.py --gpu --host            # on the GPU box
    python tools/hevc_best_mode_rate.py --ref                   # where the reference checkout is
"""
import argparse
import ctypes
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOF = 256 * 4 * 32 * 2.4e9
SIZES = {4: 262144, 8: 65536, 16: 32768, 32: 8192, 64: 2048}


def gpu(args):
    import torch

    from context_adaptive_neural_network_based_prediction_amd import _lib
    from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
    L = _lib.lib()
    ctx = ip._context(0)
    s = torch.cuda.current_stream()
    print("# GPU: pnn_hevc_best_mode_device, %s, %d warm-up + %d timed calls" % (torch.cuda.get_device_name(0), args.warmup, args.reps))
    print("%-4s %8s %-14s %10s %12s %14s %9s %14s" % ("w", "N", "outputs", "us/call", "blocks/s", "pixel-modes/s", "of roof", "lane-ops/eval"))
    g = torch.Generator(device="cuda").manual_seed(1)
    for w in args.widths:
        for n in (SIZES[w], SIZES[w] // 8):
            pats = torch.randint(0, 256, (n, 2 * w + 1, 2 * w + 1), dtype=torch.uint8, device="cuda", generator=g)
            tgts = torch.randint(0, 256, (n, w, w), dtype=torch.uint8, device="cuda", generator=g)
            idx = torch.empty(n, dtype=torch.uint8, device="cuda")
            sse = torch.empty(n, dtype=torch.int32, device="cuda")
            pred = torch.empty((n, w, w), dtype=torch.uint8, device="cuda")
            for name, pp in (("index+sse", None), ("index+sse+pred", pred.data_ptr())):
                call = lambda: L.pnn_hevc_best_mode_device(ctx, w, pats.data_ptr(), 2 * w + 1, 2 * w + 1, tgts.data_ptr(), n,
                                                           idx.data_ptr(), sse.data_ptr(), pp, None, ctypes.c_void_p(s.cuda_stream))
                for _ in range(args.warmup):
                    assert call() == 0
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                for _ in range(args.reps):
                    call()
                e1.record(s)
                e1.synchronize()
                sec = e0.elapsed_time(e1) / 1e3 / args.reps
                evals = n * 35 * w * w / sec
                print("%-4d %8d %-14s %10.1f %12.4g %14.4g %8.2f%% %14.1f" % (w, n, name, sec * 1e6, n / sec, evals,
                                                                               100 * evals / ROOF, ROOF / evals))


def host(args):
    exe = os.path.join(ROOT, "tools", "_bin", "hevc_host_rate")
    src = [os.path.join(ROOT, "tools", "hevc_host_rate.cpp"),
           os.path.join(ROOT, "context_adaptive_neural_network_based_prediction_amd", "csrc", "pnn_hevc_intra.cpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(f) > os.path.getmtime(exe) for f in src):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-O3", "-std=c++17", "-fopenmp"] + src + ["-o", exe])
    print("# host twin: pnn_hevc_intra_predict x 35 + SSE + argmin per block, %d OpenMP threads (%d CPUs visible)"
          % (args.threads, len(os.sched_getaffinity(0))))
    print("%-4s %8s %10s %12s" % ("w", "N", "seconds", "blocks/s"))
    for w in args.widths:
        n = max(4000, SIZES[w] // 2)
        out = subprocess.check_output([exe, str(w), str(n), str(args.threads)]).decode().split()
        print("%-4d %8d %10.4f %12.4g" % (w, n, float(out[3]), float(out[4])))


def ref(args):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_hevc_intra_golden as mk
    rng = np.random.default_rng(2)
    with tempfile.TemporaryDirectory() as tmp:
        rip = mk.build_reference(tmp)
        print("# reference: intraprediction.predict_series_via_hevc_best_mode (Python loop, 35 Cython calls + 35 float64 PSNRs "
              "per block), one thread")
        print("%-4s %8s %10s %12s" % ("w", "N", "seconds", "blocks/s"))
        for w in args.widths:
            n = {4: 400, 8: 400, 16: 200, 32: 50, 64: 20}[w]
            pats = rng.integers(0, 256, (n, 2 * w + 1, 2 * w + 1, 1)).astype(np.uint8)
            tgts = rng.integers(0, 256, (n, w, w, 1)).astype(np.uint8)
            t0 = time.perf_counter()
            rip.predict_series_via_hevc_best_mode(pats, tgts)
            sec = time.perf_counter() - t0
            print("%-4d %8d %10.4f %12.4g" % (w, n, sec, n / sec))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--ref", action="store_true")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--widths", type=int, nargs="+", default=[4, 8, 16, 32, 64])
    args = ap.parse_args()
    if not (args.gpu or args.host or args.ref):
        ap.error("choose at least one of --gpu, --host, --ref")
    if args.gpu:
        gpu(args)
    if args.host:
        host(args)
    if args.ref:
        ref(args)


if __name__ == "__main__":
    main()
