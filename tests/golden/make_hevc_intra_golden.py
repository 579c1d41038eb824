"""Generates tests/golden/hevc_intra_ref.npz. Run in the build container (needs /root/reference, Cython, matplotlib, PIL):

    python tests/golden/make_hevc_intra_golden.py

The reference's HEVC intra predictor (hevc/intraprediction/interface.pyx + c++/source/extracted_hevc_intraprediction.cpp) is
compiled with Cython in a temporary directory, and the reference's own hevc/intraprediction/intraprediction.py is imported
against that build (tools/tools.py from the checkout provides compute_psnr; the
C++ file is compiled with -include cmath, as it calls log() without including it).  Nothing of it is written under the repository.

What it records (data only -- inputs and expected outputs):
  mode_w{w}_m{a}x{l}_patterns / _preds
                      interface.predict_via_hevc_mode for all 35 modes, widths 4 ... 64 and masks (a, l) in
                      {(0,0), (w,0), (0,w), (4,4), (w,w)} (a = width of the above-right mask, l = height of the below-left
                      one) on seeded random patterns; for mask (0,0) also a ramp, a constant and a 0 / 255 checkerboard.
  extract_*           intraprediction.extract_intra_patterns on a seeded two-image channel stack, and the exception class
                      the reference raises for each bad-argument case named in extract_error_cases.
  best_w{w}_*         intraprediction.predict_series_via_hevc_best_mode on patterns / targets cut from seeded smooth
                      pictures, on seeded random ones, and on three edge blocks at the end: a constant pattern and target
                      (35 ties), pattern 0 / target 255 and pattern 255 / target 0 (no mode beats 0 dB).
"""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
WIDTHS = (4, 8, 16, 32, 64)


def masks(w):
    return ((0, 0), (w, 0), (0, w), (4, 4), (w, w))


def build_reference(tmp):
    """Compiles the reference's Cython interface under `tmp` and returns its intraprediction module."""
    pkg = os.path.join(tmp, "hevc", "intraprediction")
    shutil.copytree(os.path.join(REF, "hevc", "intraprediction"), pkg)
    open(os.path.join(tmp, "hevc", "__init__.py"), "w").close()
    # the C++ file calls log() without including <cmath>: newer compilers need it named on the command line
    env = dict(os.environ, CFLAGS="-include cmath")
    subprocess.check_call([sys.executable, "setup.py", "build_ext", "--inplace", "-q"], cwd=pkg, env=env,
                          stdout=subprocess.DEVNULL)
    sys.path[:0] = [tmp, REF]
    import hevc.intraprediction.intraprediction as ip
    return ip


def pattern_of(row, col):
    """A (len(col), len(row), 1) pattern that holds `row` as its first row and `col` as its first column (255 elsewhere)."""
    p = np.full((len(col), len(row), 1), 255, np.uint8)
    p[:, 0, 0] = col
    p[0, :, 0] = row
    return p


def smooth_pictures(rng, n, h, w):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    out = []
    for _ in range(n):
        a = rng.uniform(40, 215) + rng.uniform(-1.5, 1.5) * x + rng.uniform(-1.5, 1.5) * y
        a += 30 * np.sin(x / rng.uniform(4, 20) + y / rng.uniform(4, 20)) + rng.normal(0, 3, (h, w))
        out.append(np.clip(np.round(a), 0, 255))
    return np.array(out, np.uint8)[..., None]


def main():
    rng = np.random.default_rng(20261016)
    rec = {}
    with tempfile.TemporaryDirectory() as tmp:
        ip = build_reference(tmp)
        import hevc.intraprediction.interface as itf

        for w in WIDTHS:
            n_random = 3 if w <= 16 else 2 if w == 32 else 1
            for a, l in masks(w):
                h, pw = 2 * w + 1 - l, 2 * w + 1 - a
                pats = [pattern_of(rng.integers(0, 256, pw), rng.integers(0, 256, h)) for _ in range(n_random)]
                if (a, l) == (0, 0) and w <= 32:
                    ramp = np.arange(2 * w + 1) * 255 // (2 * w)
                    pats.append(pattern_of(ramp, ramp[::-1]))
                    pats.append(pattern_of(np.full(pw, 77), np.full(h, 77)))
                    pats.append(pattern_of(np.arange(pw) % 2 * 255, (np.arange(h) + 1) % 2 * 255))
                pats = np.array(pats, np.uint8)
                preds = np.array([[itf.predict_via_hevc_mode(p.copy(), w, m) for m in range(35)] for p in pats], np.uint8)
                rec["mode_w%d_m%dx%d_patterns" % (w, a, l)] = pats[..., 0]
                rec["mode_w%d_m%dx%d_preds" % (w, a, l)] = preds[..., 0]

        chans = rng.integers(0, 256, (2, 40, 48, 1)).astype(np.uint8)
        rows, cols = np.array([0, 3, 17, 23]), np.array([0, 11, 5, 31])
        rec["extract_channels"] = chans
        rec["extract_row_refs"], rec["extract_col_refs"] = rows, cols
        for a, l in ((0, 0), (8, 4)):
            rec["extract_w8_m%dx%d" % (a, l)] = ip.extract_intra_patterns(chans, 8, rows, cols, (a, l))
        cases = {
            "float_rows": lambda: ip.extract_intra_patterns(chans, 8, rows.astype(float), cols, (0, 0)),
            "float_cols": lambda: ip.extract_intra_patterns(chans, 8, rows, cols.astype(float), (0, 0)),
            "sizes_differ": lambda: ip.extract_intra_patterns(chans, 8, rows, cols[:3], (0, 0)),
            "not_uint8": lambda: ip.extract_intra_patterns(chans.astype(np.int16), 8, rows, cols, (0, 0)),
            "three_dims": lambda: ip.extract_intra_patterns(chans[..., 0], 8, rows, cols, (0, 0)),
            "two_channels": lambda: ip.extract_intra_patterns(np.concatenate([chans, chans], 3), 8, rows, cols, (0, 0)),
            "negative_row": lambda: ip.extract_intra_patterns(chans, 8, rows - 1, cols, (0, 0)),
            "negative_col": lambda: ip.extract_intra_patterns(chans, 8, rows, cols - 1, (0, 0)),
            "out_of_picture": lambda: ip.extract_intra_patterns(chans, 8, rows + 20, cols, (0, 0)),
            "mask_not_multiple_of_4": lambda: ip.extract_intra_patterns(chans, 8, rows, cols, (2, 0)),
            "mask_too_wide": lambda: ip.extract_intra_patterns(chans, 8, rows, cols, (0, 12)),
        }
        names, errors = [], []
        for name, call in cases.items():
            try:
                call()
                errors.append("")
            except Exception as e:      # the class name is the record
                errors.append(type(e).__name__)
            names.append(name)
        rec["extract_error_cases"], rec["extract_error_types"] = np.array(names), np.array(errors)

        for w in WIDTHS:
            n_smooth, n_rand = {4: 96, 8: 64, 16: 32, 32: 8, 64: 4}[w], {4: 32, 8: 16, 16: 8, 32: 4, 64: 2}[w]
            pics = smooth_pictures(rng, 2, 3 * w + 8, 3 * w + 8)
            k = n_smooth // 2
            r1 = rng.integers(0, w + 8, k)
            c1 = rng.integers(0, w + 8, k)
            mask = masks(w)[w % 5]
            pats = [ip.extract_intra_pattern(pics[i], w, r, c, (0, 0)) for i in range(2) for r, c in zip(r1, c1)]
            tgts = [pics[i, r + 1:r + 1 + w, c + 1:c + 1 + w] for i in range(2) for r, c in zip(r1, c1)]
            full = lambda p: p[:2 * w + 1 - mask[1], :2 * w + 1 - mask[0]]     # the same blocks behind a mask too
            pats = pats + [full(p) for p in pats[:n_rand]]
            tgts = tgts + tgts[:n_rand]
            pats += [pattern_of(rng.integers(0, 256, 2 * w + 1), rng.integers(0, 256, 2 * w + 1)) for _ in range(n_rand)]
            tgts += [rng.integers(0, 256, (w, w, 1)).astype(np.uint8) for _ in range(n_rand)]
            for pv, tv in ((93, 93), (0, 255), (255, 0)):
                pats.append(np.full((2 * w + 1, 2 * w + 1, 1), pv, np.uint8))
                tgts.append(np.full((w, w, 1), tv, np.uint8))
            # one array per pattern shape: the masked blocks sit in their own arrays
            for tag, sl in (("", slice(0, n_smooth)), ("_masked", slice(n_smooth, n_smooth + n_rand)),
                            ("_random", slice(n_smooth + n_rand, None))):
                P, T = np.array(pats[sl], np.uint8), np.array(tgts[sl], np.uint8)
                idx, psnr, pred = ip.predict_series_via_hevc_best_mode(P, T)
                key = "best_w%d%s" % (w, tag)
                rec[key + "_patterns"], rec[key + "_targets"] = P[..., 0], T[..., 0]
                rec[key + "_index"], rec[key + "_psnr"], rec[key + "_pred"] = idx, psnr, pred[..., 0]
            rec["best_w%d_masked_mask" % w] = np.array(mask)

    out = os.path.join(HERE, "hevc_intra_ref.npz")
    np.savez_compressed(out, **rec)
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
