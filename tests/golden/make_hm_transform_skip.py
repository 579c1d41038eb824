"""Generator of tests/golden/hm_transform_skip.npz: 4 x 4 luma units coded by HM-16.15 itself with transform_skip_flag 0 and 1, for
tests/test_hm_transform_skip.py.

    python tests/golden/make_hm_transform_skip.py /path/to/hm_16_15_regular [build directory] [output directory]

compiles tests/golden/hm_transform_skip_shim.cpp together with the tree's sources BY PATH the way tests/golden/make_hm_rdoq.py does (the
same recipe, with this shim), hands it seeded 4 x 4 residuals -- flat, one sharp edge, one sample, two-valued "text", noise, all-zero,
+-255 extremes -- at the QPs 0, 22, 37, 51, the three scans (through the intra modes 0, 26, 10), RDOQ off and on (RDOQTS equal to it, under
HM's I-slice lambda of the QP) and sign hiding off and on, and writes what HM answers.  Only the fixture is kept: recorded numbers, no code.

Layout.  residuals int16 [R][4][4]; per case c = every (residual, QP, mode, rdoq, sdh): case_residual, case_qp, case_mode, case_rdoq,
case_sdh, case_lambda (the pattern of the double), case_scan (HM's), case_abs_sum [C][2] and case_bits [C][2] (form 0: transformed,
1: skipped; bits = the increase of m_fracBits over codeCoeffNxN with the PPS flag on, 0 without a level), case_levels [C][2][4][4],
case_coeffs [C][4][4] (what xTransformSkip leaves), case_back [C][4][4] (invTransformNxN of the skipped form); flag_bits [4][2]: the
increase over codeTransformSkipFlags alone per QP of QPS, flag 0 and 1.

The generator FAILS unless HM's recorded output reaches: a unit whose skipped cbf is 0 while its transformed cbf is 1, and the reverse; a
unit where sign hiding changes a level under the flag (with RDOQ off and with RDOQ on); both forms with a level at every QP."""
import concurrent.futures
import glob
import itertools
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
import make_hm_unit_coding as unit_coding  # noqa: E402

QPS = (0, 22, 37, 51)
MODES = (0, 26, 10)                      # diagonal, horizontal, vertical scan at 4 x 4
AMPLITUDES = (1, 2, 3, 5, 9, 17, 40, 96, 255)


def residuals():
    rng = np.random.RandomState(20260)
    out = [np.zeros((4, 4), np.int64)]
    for a in AMPLITUDES:
        sign = 1 if rng.randint(2) else -1
        out.append(np.full((4, 4), sign * a))                                          # flat
        edge = np.zeros((4, 4), np.int64)
        edge[:, rng.randint(1, 4):] = sign * a
        out.append(edge if rng.randint(2) else edge.T.copy())                            # one sharp edge
        one = np.zeros((4, 4), np.int64)
        one[rng.randint(4), rng.randint(4)] = -sign * a
        out.append(one)                                                                  # one sample
        out.append(np.where(rng.randint(2, size=(4, 4)) == 1, a, -(a // 2)))             # two-valued "text"
        out.append(rng.randint(-a, a + 1, size=(4, 4)))                                  # noise
    out.append(np.where(rng.randint(2, size=(4, 4)) == 1, 255, -255))                    # extremes
    out.append(np.full((4, 4), -255))
    checker = np.full((4, 4), 255)
    checker[::2, 1::2] = -255
    checker[1::2, ::2] = -255
    out.append(checker)
    return np.array(out, np.int16)


def hm_lambda(qp):
    return 0.57 * 2.0 ** ((qp - 12) / 3.0)


def pattern(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def build(hm_tree, build_dir):
    """The recipe of make_hm_unit_coding.build with this generator's shim: the tree's TLibCommon, four encoder sources and libmd5 by
    path, what the called functions never reach left unresolved"""
    lib = os.path.join(hm_tree, "source", "Lib")
    common = os.path.join(os.path.dirname(hm_tree), "hm_common", "c++", "source_common")
    sources = [os.path.join(HERE, "hm_transform_skip_shim.cpp")] + sorted(glob.glob(os.path.join(lib, "TLibCommon", "*.cpp"))) + \
        [os.path.join(lib, "TLibEncoder", name) for name in unit_coding.ENCODER_SOURCES] + sorted(glob.glob(os.path.join(lib, "libmd5", "*.c")))
    flags = ["-O1", "-w", "-ffunction-sections", "-fdata-sections", "-I" + lib, "-I" + common, unit_coding.HM_DEFAULT_TYPES]

    def compile_one(item):
        k, source = item
        obj = os.path.join(build_dir, "%02d_%s.o" % (k, os.path.basename(source)))
        subprocess.check_call((["gcc"] if source.endswith(".c") else ["g++", "-std=c++11"]) + flags + ["-c", source, "-o", obj])
        return obj

    with concurrent.futures.ThreadPoolExecutor(8) as pool:
        objects = list(pool.map(compile_one, enumerate(sources)))
    exe = os.path.join(build_dir, "hm_transform_skip_shim")
    subprocess.check_call(["g++"] + objects + ["-Wl,--gc-sections", "-Wl,--unresolved-symbols=ignore-all", "-o", exe])
    return exe


def main():
    hm_tree = os.path.abspath(sys.argv[1])
    out_dir = sys.argv[3] if len(sys.argv) > 3 else HERE
    blocks = residuals()
    cases = list(itertools.product(range(len(blocks)), QPS, MODES, (0, 1), (0, 1)))
    lines = []
    for r, qp, mode, rdoq, sdh in cases:
        lines.append("unit %d %d %d %d %d" % (mode, qp, sdh, rdoq, pattern(hm_lambda(qp))))
        lines.append(" ".join(str(int(v)) for v in blocks[r].ravel()))
    lines += ["flag %d" % qp for qp in QPS]
    with tempfile.TemporaryDirectory() as tmp:
        build_dir = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] else tmp
        exe = build(hm_tree, build_dir)
        path = os.path.join(tmp, "cases.txt")
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
        text = subprocess.run([exe, path], stdout=subprocess.PIPE, check=True).stdout.decode()
    rows = [np.array(line.split(), np.int64) for line in text.splitlines()]
    assert len(rows) == len(cases) + len(QPS)
    units = np.array(rows[:len(cases)])
    assert units.shape == (len(cases), 5 + 64)
    assert np.abs(units[:, 5:]).max() <= 32767
    col = np.array(cases)
    arrays = {"residuals": blocks, "qps": np.array(QPS, np.uint8),
              "case_residual": col[:, 0].astype(np.int16), "case_qp": col[:, 1].astype(np.uint8), "case_mode": col[:, 2].astype(np.uint8),
              "case_rdoq": col[:, 3].astype(np.uint8), "case_sdh": col[:, 4].astype(np.uint8),
              "case_lambda": np.array([pattern(hm_lambda(c[1])) for c in cases], np.uint64), "case_scan": units[:, 0].astype(np.uint8),
              "case_abs_sum": units[:, [1, 3]].astype(np.int32), "case_bits": units[:, [2, 4]].astype(np.int64),
              "case_levels": np.stack([units[:, 5:21], units[:, 37:53]], 1).reshape(-1, 2, 4, 4).astype(np.int16),
              "case_coeffs": units[:, 21:37].reshape(-1, 4, 4).astype(np.int16), "case_back": units[:, 53:69].reshape(-1, 4, 4).astype(np.int16),
              "flag_bits": np.array(rows[len(cases):], np.int64)}
    assert arrays["flag_bits"].shape == (len(QPS), 2)

    # conditions on HM's output, not on the code under test
    cbf = arrays["case_abs_sum"] > 0
    assert set(arrays["case_scan"][col[:, 2] == 0]) == {0} and set(arrays["case_scan"][col[:, 2] == 26]) == {1} \
        and set(arrays["case_scan"][col[:, 2] == 10]) == {2}
    count = {"skipped cbf 0, transformed cbf 1": int((~cbf[:, 1] & cbf[:, 0]).sum()),
             "skipped cbf 1, transformed cbf 0": int((cbf[:, 1] & ~cbf[:, 0]).sum())}
    index = {c: i for i, c in enumerate(cases)}
    for rdoq in (0, 1):
        count["sign hiding changes a skipped level, rdoq %d" % rdoq] = sum(
            1 for (r, qp, mode, q, sdh), i in index.items()
            if q == rdoq and sdh == 1 and (arrays["case_levels"][i, 1] != arrays["case_levels"][index[(r, qp, mode, q, 0)], 1]).any())
    for qp in QPS:
        for form in (0, 1):
            count["QP %d, flag %d coded" % (qp, form)] = int((cbf[:, form] & (col[:, 1] == qp) & (arrays["case_bits"][:, form] > 0)).sum())
    print("%d cases: %s" % (len(cases), count))
    missing = [k for k, v in count.items() if v == 0]
    assert not missing, "HM's recorded output misses %s" % missing
    path = os.path.join(out_dir, "hm_transform_skip.npz")
    np.savez_compressed(path, **arrays)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
