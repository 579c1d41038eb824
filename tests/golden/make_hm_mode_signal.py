"""Generator of tests/golden/hm_mode_signal.npz: the side information of an intra luma prediction unit as HM-16.15's own functions
give it, for tests/test_hm_mode_signal.py and tests/test_gpu_mode_signal.py.

    python tests/golden/make_hm_mode_signal.py /path/to/hevc [build directory] [output directory]

`hevc` holds the trees hm_16_15_regular and hm_16_15_switch.  For each of them the generator compiles
tests/golden/hm_mode_signal_shim.cpp together with the tree's TLibCommon/*.cpp, TEncSbac.cpp, TEncBinCoderCABAC.cpp,
TEncBinCoderCABACCounter.cpp, TEncEntropy.cpp and libmd5 BY PATH (as tests/golden/make_hm_unit_coding.py does), hands it the cases
made below and records NUMBERS ONLY.  A tree that does not compile this way is left out and named in `trees`; the regular tree must.

Per tree (prefix regular_ / switch_; neighbour values V = 0 .. 34 [, 35 in the switch tree], 254 = a neighbour that is not intra,
255 = no neighbour):
  values [V]; mpm [V][V][3] and num [V][V]: uiIntraDirPred and *piMode of TComDataCU::getIntraDirPredictor for (left, above);
  triples [T][3] the distinct MPM triples in order of first appearance, triple_pair [T][2] the first (left, above) that gives each;
  bits [T][4][modes]: the increase of a TEncBinCABACCounter's m_fracBits over ONE TEncEntropy::encodeIntraDirModeLuma right after
    resetEntropy at QPs 0, 22, 37, 51, for every mode 0 .. 34 (0 .. 35 in the switch tree);
  cbf [4][2][2]: the increase over one TEncSbac::codeQtCbf for luma, [QP][transform depth][value].
NOT recorded: xModeBitsIntra's whole bits (TEncSearch is not stood up; it is getNumberOfWrittenBits of the same counter, m_fracBits >>
15) and the first-pass cost line.

The generator FAILS unless the recorded cases reach every edge of EDGES."""
import concurrent.futures
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
HM_DEFAULT_TYPES = "-DRExt__HIGH_BIT_DEPTH_SUPPORT=0"
ENCODER_SOURCES = ("TEncSbac.cpp", "TEncBinCoderCABAC.cpp", "TEncBinCoderCABACCounter.cpp", "TEncEntropy.cpp")
QPS = (0, 22, 37, 51)
TREES = (("regular", "hm_16_15_regular", 35), ("switch", "hm_16_15_switch", 36))
NOT_INTRA, NONE = 254, 255
EDGES = ("num_append 1", "num_append 2", "equal angular", "equal non-angular", "wrap at 2", "wrap at 34", "third is planar", "third is vertical",
         "third is DC", "remainder below", "remainder between", "remainder above")
SWITCH_EDGES = ("35 and angular", "35 and DC", "35 and planar", "35 twice")


def build(hm_tree, build_dir, name):
    lib = os.path.join(hm_tree, "source", "Lib")
    common = os.path.join(os.path.dirname(hm_tree), "hm_common", "c++", "source_common")
    sources = [os.path.join(HERE, "hm_mode_signal_shim.cpp")] + sorted(glob.glob(os.path.join(lib, "TLibCommon", "*.cpp"))) + \
        [os.path.join(lib, "TLibEncoder", s) for s in ENCODER_SOURCES] + sorted(glob.glob(os.path.join(lib, "libmd5", "*.c")))
    flags = ["-O1", "-w", "-ffunction-sections", "-fdata-sections", "-I" + lib, "-I" + common, "-I" + os.path.join(ROOT, "include", "tf_compat"),
             "-I" + os.path.join(ROOT, "include"), HM_DEFAULT_TYPES]

    def compile_one(item):
        k, source = item
        obj = os.path.join(build_dir, "%s_%02d_%s.o" % (name, k, os.path.basename(source)))
        subprocess.check_call((["gcc"] if source.endswith(".c") else ["g++", "-std=c++11"]) + flags + ["-c", source, "-o", obj],
                              stderr=subprocess.DEVNULL)
        return obj

    with concurrent.futures.ThreadPoolExecutor(8) as pool:
        objects = list(pool.map(compile_one, enumerate(sources)))
    exe = os.path.join(build_dir, "hm_mode_signal_shim_" + name)
    subprocess.check_call(["g++"] + objects + ["-Wl,--gc-sections", "-Wl,--unresolved-symbols=ignore-all", "-o", exe], stderr=subprocess.DEVNULL)
    return exe


def ask(exe, lines, tmp):
    cases = os.path.join(tmp, "cases.txt")
    with open(cases, "w") as f:
        f.write("\n".join(lines) + "\n")
    text = subprocess.run([exe, cases], stdout=subprocess.PIPE, check=True).stdout.decode()
    return [np.array(line.split(), np.int64) for line in text.splitlines()]


def record(exe, nb_modes, tmp):
    values = list(range(nb_modes)) + [NOT_INTRA, NONE]
    pairs = [(l, a) for l in values for a in values]
    rows = ask(exe, ["mpm %d %d" % p for p in pairs], tmp)
    assert len(rows) == len(pairs) and all(r.size == 4 for r in rows)
    v = len(values)
    mpm = np.array([r[:3] for r in rows]).reshape(v, v, 3)
    num = np.array([r[3] for r in rows]).reshape(v, v)
    assert mpm.min() >= 0 and mpm.max() < 35
    triples, first = [], []
    for pair, r in zip(pairs, rows):
        if tuple(r[:3]) not in triples:
            triples.append(tuple(r[:3]))
            first.append(pair)
    rows = ask(exe, ["bits %d %d %d %d" % (l, a, qp, nb_modes) for l, a in first for qp in QPS], tmp)
    assert len(rows) == len(first) * len(QPS) and all(r.size == nb_modes for r in rows)
    bits = np.array(rows).reshape(len(first), len(QPS), nb_modes)
    rows = ask(exe, ["cbf %d" % qp for qp in QPS], tmp)
    cbf = np.array(rows).reshape(len(QPS), 2, 2)
    assert bits.min() > 0 and bits.max() < 2 ** 31 and cbf.min() > 0
    return {"values": np.array(values, np.uint8), "mpm": mpm.astype(np.uint8), "num": num.astype(np.uint8),
            "triples": np.array(triples, np.uint8), "triple_pair": np.array(first, np.uint8), "bits": bits.astype(np.uint32),
            "cbf": cbf.astype(np.uint32)}


def reached(arrays, nb_modes):
    """The edges HM's own records show"""
    found = set()
    values = [int(x) for x in arrays["values"]]
    direction = lambda x: 1 if x >= NOT_INTRA else x
    for i, l in enumerate(values):
        for j, a in enumerate(values):
            m, num = tuple(int(x) for x in arrays["mpm"][i, j]), int(arrays["num"][i, j])
            dl, da = direction(l), direction(a)
            found.add("num_append %d" % num)
            if dl == da and 1 < dl < 35:
                found.add("equal angular")
                if m == (2, 33, 3):
                    found.add("wrap at 2")
                if m == (34, 33, 3):
                    found.add("wrap at 34")
            elif dl == da and dl < 35:
                found.add("equal non-angular")
            elif 35 in (dl, da):
                other = da if dl == 35 else dl
                found.add("35 twice" if other == 35 else "35 and angular" if other > 1 else "35 and DC" if other == 1 else "35 and planar")
            else:
                found.add({0: "third is planar", 26: "third is vertical", 1: "third is DC"}[m[2]])
    for triple, rows in zip(arrays["triples"], arrays["bits"]):
        low, mid, high = sorted(int(x) for x in triple)
        others = [m for m in range(35) if m not in (low, mid, high)]
        for name, inside in (("below", [m for m in others if m < low]), ("between", [m for m in others if low < m < high]),
                             ("above", [m for m in others if m > high])):
            if inside and len({int(rows[0][m]) for m in inside}) == 1:
                found.add("remainder " + name)
    return found


def main():
    hevc = os.path.abspath(sys.argv[1])
    out_dir = sys.argv[3] if len(sys.argv) > 3 else HERE
    arrays, stood = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        build_dir = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] else tmp
        for name, folder, nb_modes in TREES:
            try:
                exe = build(os.path.join(hevc, folder), build_dir, name)
            except subprocess.CalledProcessError:
                assert name != "regular", "the regular tree does not compile"
                continue
            got = record(exe, nb_modes, tmp)
            missing = set(EDGES + (SWITCH_EDGES if name == "switch" else ())) - reached(got, nb_modes)
            assert not missing, "%s: HM's records miss %s" % (name, sorted(missing))
            arrays.update({"%s_%s" % (name, key): value for key, value in got.items()})
            stood.append(name)
    arrays["trees"] = np.array([name in stood for name, _, _ in TREES])
    arrays["qps"] = np.array(QPS, np.uint8)
    path = os.path.join(out_dir, "hm_mode_signal.npz")
    np.savez_compressed(path, **arrays)
    print("%s: %d bytes, trees %s" % (path, os.path.getsize(path), stood))


if __name__ == "__main__":
    main()
