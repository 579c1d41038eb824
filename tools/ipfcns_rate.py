"""IPFCN-S rate record -> profiles/ipfcns_rate.txt.

Per width and N (1, 64, 1024, 8192; at most 2048 at w = 32): device-resident blocks/s of pnn_ipfcns_forward_device (rows and
outputs already on the GPU, median of timed repetitions) and its TFLOP/s against the 157.3 TF f32 MFMA roof of one MI355X;
torch's own f32 chain (F.linear + F.prelu, TF32 off) on the same device and inputs as a yardstick; the host twin
pnn_ipfcns_forward_host on 16 threads.  `--prof` runs only the fused path (pnn_ipfcns_predict_device) in a loop, for
`rocprofv3 --kernel-trace --stats`; `--share DIR` reads that run's kernel_stats.csv and appends the share of the gather, PReLU
and epilogue kernels to the record.

    python tools/ipfcns_rate.py [--out profiles/ipfcns_rate.txt]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/ipfcns_rate.py --prof
    python tools/ipfcns_rate.py --share DIR [--out ...]
"""
import argparse
import csv
import glob
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOF_TF = 157.3


def params_for(w, seed):
    from context_adaptive_neural_network_based_prediction_amd import ipfcns as I
    K, H, O = I.layer_dims(w)
    rng = np.random.default_rng(seed)
    s = (0.032 * np.sqrt(192 / K), 0.0188 * np.sqrt(512 / H), 0.0168 * np.sqrt(512 / H), 0.092 * np.sqrt(512 / H))
    dims = (K, H, H, H, O)
    parts = []
    for l in range(4):
        parts.append(rng.normal(0, s[l], dims[l + 1] * dims[l]))
        parts.append(rng.normal(0, 0.02, dims[l + 1]))
        if l < 3:
            parts.append(rng.uniform(-0.3, 0.6, dims[l + 1]))
    return np.concatenate(parts).astype(np.float32)


def flops_per_block(w):
    from context_adaptive_neural_network_based_prediction_amd import ipfcns as I
    K, H, O = I.layer_dims(w)
    return 2.0 * (K * H + 2 * H * H + H * O)


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    return float(np.median(ts))


def torch_chain(params, w):
    import torch
    import torch.nn.functional as F
    from context_adaptive_neural_network_based_prediction_amd import ipfcns as I
    K, H, O = I.layer_dims(w)
    dims = (K, H, H, H, O)
    t = torch.from_numpy(params).cuda()
    layers, o = [], 0
    for l in range(4):
        W = t[o:o + dims[l + 1] * dims[l]].view(dims[l + 1], dims[l]); o += dims[l + 1] * dims[l]
        b = t[o:o + dims[l + 1]]; o += dims[l + 1]
        a = None
        if l < 3:
            a = t[o:o + dims[l + 1]]; o += dims[l + 1]
        layers.append((W, b, a))

    def run(x):
        h = x
        for W, b, a in layers:
            h = F.linear(h, W, b)
            if a is not None:
                h = F.prelu(h, a)
        return h
    return run


def record(out):
    import torch
    from context_adaptive_neural_network_based_prediction_amd import ipfcns as I
    torch.backends.cuda.matmul.allow_tf32 = False
    lines = ["# IPFCN-S rates on one MI355X (tools/ipfcns_rate.py): device-resident fc1..fc4 (pnn_ipfcns_forward_device, exact-f32",
             "# order), torch's F.linear + F.prelu f32 chain (TF32 off) on the same inputs, the host twin on 16 threads.",
             "# TF/s = 2 (KH + 2H^2 + Hw^2) N / t; roof 157.3 TF (f32 MFMA).",
             "%-4s %-6s %14s %9s %7s %14s %9s %9s %14s" % ("w", "N", "lib blocks/s", "lib us", "%roof", "torch blocks/s",
                                                            "torch us", "lib/torch", "twin blocks/s")]
    for w in I.WIDTHS:
        params = params_for(w, 7 + w)
        net = I.NetIpfcns(w, params)
        chain = torch_chain(params, w)
        for n in (1, 64, 1024, 8192):
            if w == 32 and n > 2048:
                n = 2048
            x = torch.from_numpy(np.random.default_rng(w + n).normal(0, 40, (n, I.input_size(w))).astype(np.float32)).cuda()
            reps = 50 if n <= 1024 else 20
            t_lib = timed(lambda: net.forward_device(x), reps)
            t_torch = timed(lambda: chain(x), reps)
            xh = x[:min(n, 1024)].cpu().numpy()
            t0 = time.perf_counter()
            I.forward_host(params, w, xh)
            t_twin = time.perf_counter() - t0
            lines.append("%-4d %-6d %14.0f %9.1f %7.2f %14.0f %9.1f %9.2f %14.0f" % (
                w, n, n / t_lib, t_lib * 1e6, 100 * flops_per_block(w) * n / t_lib / 1e12 / ROOF_TF, n / t_torch, t_torch * 1e6,
                t_torch / t_lib, xh.shape[0] / t_twin))
            print(lines[-1], flush=True)
        net.close()
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


def prof():
    import torch
    from context_adaptive_neural_network_based_prediction_amd import ipfcns as I
    for w in I.WIDTHS:
        net = I.NetIpfcns(w, params_for(w, 7 + w))
        span = 2 * w + 8
        rng = np.random.default_rng(w)
        img = torch.from_numpy(rng.integers(0, 256, (1, 8 * span, 8 * span)).astype(np.uint8)).cuda()
        n = 2048 if w == 32 else 8192
        rows = torch.from_numpy(rng.integers(0, 7 * span, n).astype(np.int32)).cuda()
        cols = torch.from_numpy(rng.integers(0, 7 * span, n).astype(np.int32)).cuda()
        tg = torch.from_numpy(rng.integers(0, 256, (n, w, w)).astype(np.uint8)).cuda()
        for _ in range(10):
            net.predict_from_channels_device(img, rows, cols, tg)
        net.close()


def share(d, out):
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit("no kernel_stats.csv under %s" % d)
    tot, part = 0.0, {}
    with open(files[0]) as f:
        for row in csv.DictReader(f):
            ns = float(row.get("TotalDurationNs") or float(row["AverageNs"]) * float(row["Calls"]))
            name = row["Name"]
            tot += ns
            for k in ("ipfcns_gather", "ipfcns_prelu", "ipfcns_epilogue"):
                if k in name:
                    part[k] = part.get(k, 0.0) + ns
    lines = ["", "# rocprofv3 --kernel-trace --stats of the fused path (pnn_ipfcns_predict_device, 10 calls per width, N = 8192;",
             "# 2048 at w = 32; all widths in one trace): share of the non-GEMM kernels in the kernel time"]
    for k in ("ipfcns_gather", "ipfcns_prelu", "ipfcns_epilogue"):
        lines.append("%-18s %8.3f ms  %6.2f %%" % (k, part.get(k, 0.0) * 1e-6, 100 * part.get(k, 0.0) / tot))
    s = sum(part.values())
    lines.append("%-18s %8.3f ms  %6.2f %%   (all kernels %.3f ms)" % ("non-GEMM total", s * 1e-6, 100 * s / tot, tot * 1e-6))
    with open(out, "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ipfcns_rate.txt"))
    ap.add_argument("--prof", action="store_true")
    ap.add_argument("--share", default=None)
    a = ap.parse_args()
    if a.prof:
        prof()
    elif a.share:
        share(a.share, a.out)
    else:
        record(a.out)
