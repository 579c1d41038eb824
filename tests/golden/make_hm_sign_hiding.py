"""Generator of tests/golden/hm_sign_hiding.npz: recorded calls of HM-16.15's own TComTrQuant::signBitHidingHDQ, the sign-data hiding of
xQuant with RDOQ 0, for tests/test_sign_hiding.py.

    python tests/golden/make_hm_sign_hiding.py /path/to/hm_16_15_regular [build directory]

compiles tests/golden/hm_sign_hiding_shim.cpp together with the tree's TComTrQuant.cpp and TComRom.cpp BY PATH into the build directory
(a temporary one by default; what the called functions never reach stays unresolved and unreferenced), hands it the cases made below
and writes the fixture.  Only the fixture is kept: numbers, no code.

Per unit size T and scan the size allows (0 diagonal, 1 horizontal, 2 vertical; diagonal only above 8 x 8), K records: 'coef_T_s' (pCoef),
'before_T_s' (pQCoef in), 'delta_u_T_s' (deltaU, int16) and 'after_T_s' (pQCoef out), int32 [K, T, T].  The inputs are made here, not by a
quantiser: the function takes them as they come, and so must the host entry.  The cases:
  sparse and dense random levels (groups whose parity is right and wrong alike; the last group with zeros above its last level; zero
  positions below the first level whose coefficients have either sign); remainders from three values only (ties); levels of +-1 with
  remainders <= 0 (the first level must not go to zero); a unit whose first group -- not the last one, a later group has a level --
  has its cheapest change at a zero of a high position; levels of 32767 and -32768, which may only come down.

WHAT IS PINNED: signBitHidingHDQ itself.  WHAT IS NOT, HERE: the line of xQuant that makes deltaU and codeCoeffNxN's rule that the hidden
sign is not coded; both are pinned by tests/golden/make_hm_unit_coding.py, which runs transformNxN and codeCoeffNxN on whole units."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HM_DEFAULT_TYPES = "-DRExt__HIGH_BIT_DEPTH_SUPPORT=0"
SIZES = (4, 8, 16, 32)


def build(hm_tree, build_dir):
    lib = os.path.join(hm_tree, "source", "Lib")
    exe = os.path.join(build_dir, "hm_sign_hiding_shim")
    subprocess.check_call(["g++", "-O1", "-w", "-std=c++11", "-ffunction-sections", "-fdata-sections", "-I" + lib, HM_DEFAULT_TYPES,
                           os.path.join(HERE, "hm_sign_hiding_shim.cpp")] +
                          [os.path.join(lib, "TLibCommon", name) for name in ("TComTrQuant.cpp", "TComRom.cpp")] +
                          ["-Wl,--gc-sections", "-Wl,--unresolved-symbols=ignore-all", "-o", exe])
    return exe


def with_signs(rng, levels, zero_coef=40):
    """Coefficients that go with levels: the level's sign where there is one, a small value of either sign elsewhere"""
    t = levels.shape[0]
    small = rng.integers(-zero_coef, zero_coef + 1, (t, t))
    return np.where(levels != 0, levels * 37 + np.sign(levels) * rng.integers(0, 30, (t, t)), small)


def cases_of(t, seed):
    """[(coef, levels, delta_u)] int64 [T, T]"""
    rng = np.random.default_rng(seed)
    out = []

    def add(levels, delta_u, coef=None):
        out.append((with_signs(rng, levels) if coef is None else coef, levels, delta_u))

    remainder = lambda: rng.integers(-86, 171, (t, t))  # noqa: E731
    for density in (0.05, 0.15, 0.4, 0.4, 0.8, 1.0, 1.0) if t < 32 else (0.05, 0.4, 1.0):    # sparse to dense, small levels: both parities
        levels = np.where(rng.random((t, t)) < density, rng.integers(-3, 4, (t, t)), 0)
        add(levels, remainder())
    add(rng.integers(-300, 301, (t, t)), remainder())                            # dense and large
    for density in (0.3, 1.0):                                                   # ties: three remainders only
        levels = np.where(rng.random((t, t)) < density, rng.integers(-2, 3, (t, t)), 0)
        add(levels, rng.choice(np.array([-3, 0, 5]), (t, t)))
    add(np.where(rng.random((t, t)) < 0.6, rng.choice(np.array([-1, 1]), (t, t)), 0), rng.integers(-86, 1, (t, t)))   # +-1, remainders <= 0
    add(rng.choice(np.array([-1, 1]), (t, t)), np.zeros((t, t), np.int64))       # all +-1, all remainders 0: every first level is forbidden
    # the first group's cheapest change is the zero at its highest scan position; at T > 4 a later group holds a level, so the first
    # group is not the last one and all its 16 positions are candidates (at T = 4 the one group is the last: the candidates end at `last`)
    levels = np.zeros((t, t), np.int64)
    levels[0, 0], levels[0, 1], levels[1, 0], levels[1, 1], levels[0, 2], levels[2, 0] = 2, -1, 1, 3, 1, -2
    delta_u = np.full((t, t), 1, np.int64)
    delta_u[3, 3] = 150
    levels[t - 1, t - 1] = 1 if t > 4 else 0
    for flip in (1, -1):
        add(levels * flip, delta_u)
    extreme = rng.choice(np.array([32767, -32768, 32767, -32768, 1, -1, 0]), (t, t))       # may only come down
    add(extreme, remainder())
    add(np.full((t, t), 32767), np.full((t, t), 9, np.int64))
    add(np.full((t, t), -32768), remainder(), coef=np.full((t, t), -32768 * 3))
    return out


def main():
    hm_tree = sys.argv[1]
    records = {}
    lines = []
    for t in SIZES:
        for scan in ((0, 1, 2) if t <= 8 else (0,)):
            records[(t, scan)] = cases_of(t, 100 * t + scan)
            for arrays in records[(t, scan)]:
                lines.append("%d %d" % (t, scan))
                lines.extend(" ".join(str(int(v)) for v in a.ravel()) for a in arrays)
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(hm_tree, sys.argv[2] if len(sys.argv) > 2 else tmp)
        cases = os.path.join(tmp, "cases.txt")
        with open(cases, "w") as f:
            f.write("\n".join(lines) + "\n")
        text = subprocess.run([exe, cases], stdout=subprocess.PIPE, check=True).stdout.decode()
    after = iter(text.splitlines())
    arrays = {}
    for (t, scan), cases in records.items():
        for k, name in enumerate(("coef", "before", "delta_u")):
            arrays["%s_%d_%d" % (name, t, scan)] = np.array([c[k] for c in cases], np.int16 if name == "delta_u" else np.int32)
        arrays["after_%d_%d" % (t, scan)] = np.array([[int(v) for v in next(after).split()] for _ in cases], np.int32).reshape(-1, t, t)
    assert next(after, None) is None
    path = os.path.join(HERE, "hm_sign_hiding.npz")
    np.savez_compressed(path, **arrays)
    changed = sum(int((arrays["after_%d_%d" % key] != arrays["before_%d_%d" % key]).sum()) for key in records)
    print("%s: %d bytes, %d records, %d changed levels" % (path, os.path.getsize(path), sum(len(c) for c in records.values()), changed))


if __name__ == "__main__":
    main()
