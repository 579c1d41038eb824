"""Generator of tests/golden/hm_rdoq.npz: transform units quantised by HM-16.15's own xRateDistOptQuant, for tests/test_hm_rdoq.py and
tests/test_gpu_rdoq.py.

    python tests/golden/make_hm_rdoq.py /path/to/hm_16_15_regular [build directory] [output directory]

compiles tests/golden/hm_rdoq_shim.cpp together with the tree's sources BY PATH the way tests/golden/make_hm_unit_coding.py does (the
same recipe, with this shim), hands it the cases of tests/hm_rdoq_cases.py and writes the fixture (layout and edges: that module).
Only the fixture is kept: recorded numbers, no code.  The generator FAILS unless HM's recorded output reaches every edge of
hm_rdoq_cases.wanted_edges at every T, and prints the number of cases that reach each."""
import concurrent.futures
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
import make_hm_unit_coding as unit_coding  # noqa: E402
from tests import hm_rdoq_cases as rq  # noqa: E402
from tests import hm_unit_cases as units  # noqa: E402


def build(hm_tree, build_dir):
    """The recipe of make_hm_unit_coding.build with this generator's shim: the tree's TLibCommon, four encoder sources and libmd5 by
    path, what the called functions never reach left unresolved"""
    lib = os.path.join(hm_tree, "source", "Lib")
    common = os.path.join(os.path.dirname(hm_tree), "hm_common", "c++", "source_common")
    sources = [os.path.join(HERE, "hm_rdoq_shim.cpp")] + sorted(glob.glob(os.path.join(lib, "TLibCommon", "*.cpp"))) + \
        [os.path.join(lib, "TLibEncoder", name) for name in unit_coding.ENCODER_SOURCES] + sorted(glob.glob(os.path.join(lib, "libmd5", "*.c")))
    flags = ["-O1", "-w", "-ffunction-sections", "-fdata-sections", "-I" + lib, "-I" + common, unit_coding.HM_DEFAULT_TYPES]

    def compile_one(item):
        k, source = item
        obj = os.path.join(build_dir, "%02d_%s.o" % (k, os.path.basename(source)))
        subprocess.check_call((["gcc"] if source.endswith(".c") else ["g++", "-std=c++11"]) + flags + ["-c", source, "-o", obj])
        return obj

    with concurrent.futures.ThreadPoolExecutor(8) as pool:
        objects = list(pool.map(compile_one, enumerate(sources)))
    exe = os.path.join(build_dir, "hm_rdoq_shim")
    subprocess.check_call(["g++"] + objects + ["-Wl,--gc-sections", "-Wl,--unresolved-symbols=ignore-all", "-o", exe])
    return exe


def main():
    from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
    hm_tree = os.path.abspath(sys.argv[1])
    out_dir = sys.argv[3] if len(sys.argv) > 3 else HERE
    lines, pairs = [], {}
    for t in rq.SIZES:
        pairs[t] = rq.pairs_of(t)
        predictions, targets, modes = pairs[t]
        for p, qp, f, sdh, depth in rq.cases_of(t):
            lam = rq.lambda_of_case(t, (p, qp, f, sdh, depth))
            lines.append("unit %d %d %d %d %d %d" % (t, modes[p], qp, sdh, depth, units.pattern(lam)))
            lines.append(" ".join(str(int(v)) for v in (targets[p].astype(np.int64) - predictions[p].astype(np.int64)).ravel()))
        for qp in rq.QPS:
            lines.append("est %d %d 0" % (t, qp))
    with tempfile.TemporaryDirectory() as tmp:
        build_dir = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] else tmp
        exe = build(hm_tree, build_dir)
        cases = os.path.join(tmp, "cases.txt")
        with open(cases, "w") as f:
            f.write("\n".join(lines) + "\n")
        text = subprocess.run([exe, cases], stdout=subprocess.PIPE, check=True).stdout.decode()
    answers = iter(text.splitlines())
    arrays = {}
    for t in rq.SIZES:
        predictions, targets, modes = pairs[t]
        mine = rq.cases_of(t)
        rows = [np.array(next(answers).split(), np.int64) for _ in mine]
        assert all(row.size == 4 + 2 * t * t for row in rows)
        arrays.update({"pair_predictions_%d" % t: predictions, "pair_targets_%d" % t: targets, "pair_modes_%d" % t: modes,
                       "case_pair_%d" % t: np.array([c[0] for c in mine], np.int16), "case_qp_%d" % t: np.array([c[1] for c in mine], np.uint8),
                       "case_factor_%d" % t: np.array([c[2] for c in mine], np.uint8), "case_sdh_%d" % t: np.array([c[3] for c in mine], np.uint8),
                       "case_depth_%d" % t: np.array([c[4] for c in mine], np.uint8),
                       "case_lambda_%d" % t: np.array([units.pattern(rq.lambda_of_case(t, c)) for c in mine], np.uint64),
                       "case_scan_%d" % t: np.array([r[0] for r in rows], np.uint8), "case_abs_sum_%d" % t: np.array([r[1] for r in rows], np.int32),
                       "case_bits_%d" % t: np.array([r[2] for r in rows], np.int64), "case_cbf_ctx_%d" % t: np.array([r[3] for r in rows], np.uint8)})
        for name, start in (("levels", 4), ("residual", 4 + t * t)):
            block = np.array([r[start:start + t * t] for r in rows]).reshape(-1, t, t)
            assert block.min() >= -32768 and block.max() <= 32767
            arrays["case_%s_%d" % (name, t)] = block.astype(np.int16)
        est = np.array([next(answers).split() for _ in rq.QPS], np.int32)
        assert est.shape == (len(rq.QPS), rq.EST_WORDS)
        arrays["est_bits_%d" % t] = est
    assert next(answers, None) is None
    for t in rq.SIZES:                                    # conditions on HM's output, not on the code under test
        count = rq.reached(arrays, t)
        print("T %d, %d cases: %s" % (t, len(rq.cases_of(t)), dict(sorted(count.items()))))
        missing = rq.wanted_edges(t) - set(count)
        assert not missing, "T %d: HM's recorded output misses %s" % (t, sorted(missing))
    path = os.path.join(out_dir, "hm_rdoq.npz")
    np.savez_compressed(path, **arrays)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
