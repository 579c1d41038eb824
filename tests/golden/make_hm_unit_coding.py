"""Generator of tests/golden/hm_unit_coding.npz: WHOLE transform units coded by HM-16.15's own functions, for
tests/test_hm_unit_coding.py and tests/test_gpu_hm_unit_coding.py.

    python tests/golden/make_hm_unit_coding.py /path/to/hm_16_15_regular [build directory] [output directory]

compiles tests/golden/hm_unit_coding_shim.cpp together with the tree's TLibCommon/*.cpp, TEncSbac.cpp, TEncBinCoderCABAC.cpp,
TEncBinCoderCABACCounter.cpp, TEncEntropy.cpp and libmd5 BY PATH into the build directory (a temporary one by default; what the called
functions never reach stays unresolved and unreferenced), hands it the cases made below and writes the fixture (layout:
tests/hm_unit_cases.py).  Only the fixture is kept: recorded numbers, no code.  The shim stands up one TComSPS / TComPPS / TComSlice and a
TComPic of one CTU, so that a TComDataCU and a TComTURecurse exist for one intra luma coding unit with one transform unit of T x T:
4:0:0, 8 bit, I slice, SliceQp = the QP, RDOQ 0, flat quantisation, no transform skip / transquant bypass / range-extension tool.  The
tree is compiled with RExt__HIGH_BIT_DEPTH_SUPPORT 0, HM's documented default, as tests/golden/make_hm_transforms.py explains: the
standard's 6-bit matrices in the forward transform too.

WHAT IS PINNED, per case (a (prediction, target) pair with its intra mode, at a QP, SignDataHidingEnabledFlag off or on):
  TComTrQuant::transformNxN on the residual: the levels after xQuant -- its quantisation, its remainder deltaU and the hand-over to
    signBitHidingHDQ included -- and uiAbsSum;
  the scan HM chose for the unit (getTUEntropyCodingParameters' scanType), and TComDataCU::getCoefScanIdx for EVERY mode 0 .. 34 at every T;
  the increase of a TEncBinCABACCounter's m_fracBits over ONE TEncSbac::codeCoeffNxN call right after resetEntropy at that QP: the order
    of the syntax elements, the inferred flags, the c1 walk, the Rice parameter, the escape codes, the hidden sign -- also on given
    levels of +-32767 / -32768, which 8-bit residuals cannot produce;
  TComTrQuant::invTransformNxN on those levels: the reconstructed residual;
  TComRdCost::calcRdCost(bits, distortion, DF_DEFAULT) after setLambda, as 64-bit patterns, on (lambda, D, R) triples that include ones
    for which a fused multiply-add gives another double, and on the winners of one second-pass call of the host twin under four of
    those lambdas (the triples that call reaches; HM is asked for their costs, nothing of the twin's is recorded as a result).
WHAT IS NOT: lambda itself.  TEncSlice::calculateLambda sits too deep in the encoder to be called alone; the lambdas here are
intraprediction.hm_intra_lambda's at QPs 0 .. 51, this project's restatement of it.  Nor cbf_luma, mode bits, the running contexts of a
slice (every unit starts from resetEntropy) or RDOQ.

The pairs: the extremes, random and smooth pairs of tests/trquant_cases.py, each coded at QPs 0, 22, 37, 51 with the flag off and on;
and pairs built BACKWARDS from wanted level patterns (dequantised by the numpy restatement, inverse-transformed, added to a flat
prediction), each at the one QP it was built for, flag off and on.  The generator FAILS unless HM's recorded levels reach every edge of
tests/hm_unit_cases.wanted_edges at every T."""
import concurrent.futures
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import cabac_rate_cases as cabac  # noqa: E402
from tests import hm_unit_cases as units  # noqa: E402
from tests import trquant_cases as tq  # noqa: E402

HM_DEFAULT_TYPES = "-DRExt__HIGH_BIT_DEPTH_SUPPORT=0"
ENCODER_SOURCES = ("TEncSbac.cpp", "TEncBinCoderCABAC.cpp", "TEncBinCoderCABACCounter.cpp", "TEncEntropy.cpp")


def build(hm_tree, build_dir):
    lib = os.path.join(hm_tree, "source", "Lib")
    common = os.path.join(os.path.dirname(hm_tree), "hm_common", "c++", "source_common")      # tools.h, which the tree's TEncSearch.h includes
    sources = [os.path.join(HERE, "hm_unit_coding_shim.cpp")] + sorted(glob.glob(os.path.join(lib, "TLibCommon", "*.cpp"))) + \
        [os.path.join(lib, "TLibEncoder", name) for name in ENCODER_SOURCES] + sorted(glob.glob(os.path.join(lib, "libmd5", "*.c")))
    flags = ["-O1", "-w", "-ffunction-sections", "-fdata-sections", "-I" + lib, "-I" + common, HM_DEFAULT_TYPES]

    def compile_one(item):
        k, source = item
        obj = os.path.join(build_dir, "%02d_%s.o" % (k, os.path.basename(source)))
        subprocess.check_call((["gcc"] if source.endswith(".c") else ["g++", "-std=c++11"]) + flags + ["-c", source, "-o", obj])
        return obj

    with concurrent.futures.ThreadPoolExecutor(8) as pool:
        objects = list(pool.map(compile_one, enumerate(sources)))
    exe = os.path.join(build_dir, "hm_unit_coding_shim")
    subprocess.check_call(["g++"] + objects + ["-Wl,--gc-sections", "-Wl,--unresolved-symbols=ignore-all", "-o", exe])
    return exe


def pairs_of(t):
    """(predictions, targets [n, T, T], modes [n], qps per pair): the base pairs at every QP, then the backwards pairs at their own"""
    predictions, targets = tq.mixed_pairs(t, units.NB_BASE_PAIRS[t], 7000 + t)
    predictions, targets = list(predictions), list(targets)
    modes = [units.MODES[k % len(units.MODES)] for k in range(len(predictions))]        # at T = 4 and 8: every mode of the list
    qps = [units.QPS] * len(predictions)
    for _, mode, levels in units.wanted_patterns(t):
        made = units.backwards(levels)
        assert made is not None, "a wanted pattern fits no QP"
        predictions.append(made[0]), targets.append(made[1]), modes.append(mode), qps.append((made[2],))
    return np.array(predictions), np.array(targets), np.array(modes, np.uint8), qps


def given_levels(t):
    """[(levels, mode, qp, flag)] for codeCoeffNxN alone: the extreme sets of cabac_rate_cases.level_sets and two ordinary ones"""
    sets = cabac.level_sets(t, 9100 + t)
    out = []
    for k, index in enumerate((6, 7, 8, 6, 7, 8, 5, 3)):
        mode = (0, 26, 10)[k % 3] if t <= 8 else 0
        out.append((sets[index], mode, units.QPS[(k + index) % 4], k % 2))
    return out


def cost_triples(rng):
    """(lambda, D, R) float / int lists: lambdas of QPs 0 .. 51; every tenth or so differs under a fused multiply-add, at least 64 do"""
    from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
    lams = [ip.hm_intra_lambda(qp) for qp in range(52)]
    plain, differing = [], []
    for lam in lams:                                      # the corners: no bits, no distortion, the largest of both
        plain += [(lam, 0, 0), (lam, 12345, 0), (lam, 0, 77), (lam, 2 ** 32 - 1, 2 ** 24)]
    while len(differing) < 64 or len(plain) < 52 * 6:
        lam = lams[int(rng.integers(0, 52))]
        d, r = int(rng.integers(0, 1 << int(rng.integers(4, 29)))), int(rng.integers(0, 1 << int(rng.integers(2, 21))))
        if units.fused(lam, d, r) != np.float64(d) + np.float64(lam) * np.float64(r):
            if len(differing) < 64:
                differing.append((lam, d, r))
        elif len(plain) < 52 * 6:
            plain.append((lam, d, r))
    return plain + differing


def second_pass_triples(lambdas):
    """The winners' (lambda, D, R) of the host twin's second pass on rd_pass_cases.seeded, R in whole bits"""
    from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
    from tests import rd_pass_cases
    out = []
    for flag in (False, True):
        res = ip.rd_pass(*rd_pass_cases.seeded(units.RD_WIDTH, units.RD_BLOCKS), units.RD_QPS, sign_data_hiding=flag, lambdas=lambdas)
        for qi, lam in enumerate(lambdas):
            out += [(lam, int(d), int(r) >> 15) for d, r in zip(res['sses'][qi], res['rates'][qi])]
    return sorted(set(out))


def main():
    hm_tree = os.path.abspath(sys.argv[1])
    out_dir = sys.argv[3] if len(sys.argv) > 3 else HERE
    lines, layout = [], []

    def record(word, t, mode, qp, flag, values):
        lines.append("%s %d %d %d %d" % (word, t, mode, qp, flag))
        lines.append(" ".join(str(int(v)) for v in np.asarray(values).ravel()))

    pairs, calls = {}, {}
    for t in units.SIZES:
        pairs[t] = pairs_of(t)
        predictions, targets, modes, qps = pairs[t]
        for p in range(len(modes)):
            for qp in qps[p]:
                for flag in (0, 1):
                    record("unit", t, modes[p], qp, flag, targets[p].astype(np.int64) - predictions[p].astype(np.int64))
                    layout.append((t, p, qp, flag))
        calls[t] = given_levels(t)
        for levels, mode, qp, flag in calls[t]:
            record("code", t, mode, qp, flag, levels)
    lines.append("scans")
    triples = cost_triples(np.random.default_rng(52))
    differs = [units.fused(*tr) != np.float64(tr[1]) + np.float64(tr[0]) * np.float64(tr[2]) for tr in triples]
    rd_lambdas = []
    for tr, differ in zip(triples, differs):              # four distinct lambdas of triples that differ under a fused multiply-add
        if differ and tr[0] not in rd_lambdas and len(rd_lambdas) < 4:
            rd_lambdas.append(tr[0])
    rd_lambdas.sort()
    rd_first = len(triples)
    triples += second_pass_triples(rd_lambdas)
    differs += [units.fused(*tr) != np.float64(tr[1]) + np.float64(tr[0]) * np.float64(tr[2]) for tr in triples[rd_first:]]
    assert any(differs[rd_first:]), "no winner of the second-pass call differs under a fused multiply-add"
    for lam, d, r in triples:
        lines.append("cost %d %d %d" % (units.pattern(lam), d, r))

    with tempfile.TemporaryDirectory() as tmp:
        build_dir = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] else tmp
        exe = build(hm_tree, build_dir)
        cases = os.path.join(tmp, "cases.txt")
        with open(cases, "w") as f:
            f.write("\n".join(lines) + "\n")
        text = subprocess.run([exe, cases], stdout=subprocess.PIPE, check=True).stdout.decode()
    answers = iter(text.splitlines())
    arrays = {}
    done = 0
    for t in units.SIZES:
        predictions, targets, modes, _ = pairs[t]
        mine = [entry for entry in layout if entry[0] == t]
        rows = [np.array(next(answers).split(), np.int64) for _ in mine]
        done += len(mine)
        assert all(row.size == 3 + 2 * t * t for row in rows)
        arrays.update({"pair_predictions_%d" % t: predictions, "pair_targets_%d" % t: targets, "pair_modes_%d" % t: modes,
                       "case_pair_%d" % t: np.array([e[1] for e in mine], np.int16), "case_qp_%d" % t: np.array([e[2] for e in mine], np.uint8),
                       "case_sdh_%d" % t: np.array([e[3] for e in mine], np.uint8), "case_scan_%d" % t: np.array([r[0] for r in rows], np.uint8),
                       "case_abs_sum_%d" % t: np.array([r[1] for r in rows], np.int32), "case_bits_%d" % t: np.array([r[2] for r in rows], np.int64)})
        for name, start in (("levels", 3), ("residual", 3 + t * t)):
            block = np.array([r[start:start + t * t] for r in rows]).reshape(-1, t, t)
            assert block.min() >= -32768 and block.max() <= 32767
            arrays["case_%s_%d" % (name, t)] = block.astype(np.int16)
        rows = [np.array(next(answers).split(), np.int64) for _ in calls[t]]
        arrays.update({"code_levels_%d" % t: np.array([c[0] for c in calls[t]], np.int16), "code_mode_%d" % t: np.array([c[1] for c in calls[t]], np.uint8),
                       "code_qp_%d" % t: np.array([c[2] for c in calls[t]], np.uint8), "code_sdh_%d" % t: np.array([c[3] for c in calls[t]], np.uint8),
                       "code_scan_%d" % t: np.array([r[0] for r in rows], np.uint8), "code_bits_%d" % t: np.array([r[1] for r in rows], np.int64)})
    arrays["scan_of_mode"] = np.array(next(answers).split(), np.uint8).reshape(4, 35)
    arrays.update({"cost_lambda": np.array([units.pattern(tr[0]) for tr in triples], np.uint64), "cost_d": np.array([tr[1] for tr in triples], np.uint32),
                   "cost_r": np.array([tr[2] for tr in triples], np.uint64), "cost_j": np.array([int(next(answers)) for _ in triples], np.uint64),
                   "cost_fused_differs": np.array(differs), "rd_lambdas": np.array([units.pattern(v) for v in rd_lambdas], np.uint64),
                   "rd_first": np.array(rd_first, np.int64)})
    assert next(answers, None) is None
    for t in units.SIZES:                                 # conditions on HM's output, not on the code under test
        missing = units.wanted_edges(t) - units.reached(arrays, t)
        assert not missing, "T %d: HM's recorded levels miss %s" % (t, sorted(missing))
    path = os.path.join(out_dir, "hm_unit_coding.npz")
    np.savez_compressed(path, **arrays)
    print("%s: %d bytes, %d units, %d calls on given levels, %d cost triples (%d differ under a fused multiply-add)" % (
        path, os.path.getsize(path), done, sum(len(c) for c in calls.values()), len(triples), sum(differs)))


if __name__ == "__main__":
    main()
