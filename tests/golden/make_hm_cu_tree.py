"""Generator of tests/golden/hm_cu_tree.npz: the bins of the coding tree as HM-16.15 itself counts them, for tests/test_hm_cu_tree.py.

    python tests/golden/make_hm_cu_tree.py /path/to/hm_16_15_regular [build directory] [output directory]

compiles tests/golden/hm_cu_tree_shim.cpp together with the tree's sources BY PATH the way tests/golden/make_hm_transform_skip.py does
(the same recipe, with this shim) and writes what HM answers.  Only the fixture is kept: recorded numbers, no code.

Layout.  split_bits int64 [52][3][2]: the increase of m_fracBits over TEncSbac::codeSplitFlag at QP 0 .. 51, context 0 .. 2, flag 0 / 1,
from the states an I slice of the QP starts with; part_bits int64 [52][2]: the same over codePartSize of an intra CU of the minimum size,
[0] SIZE_NxN (bin 0) and [1] SIZE_2Nx2N (bin 1); split_ctx uint8 [4][4]: TComDataCU::getCtxSplitFlag by the state of the left and of the
above neighbour, 0 absent, 1 shallower, 2 equal, 3 deeper -- asked of a CU with real neighbours inside one CTU.

The generator FAILS unless both bin values were recorded for every context at every QP and the whole truth table was."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
import make_hm_transform_skip as recipe  # noqa: E402


def build(hm_tree, build_dir):
    """make_hm_transform_skip.build with this generator's shim in the other's place"""
    import glob
    import concurrent.futures
    unit_coding = recipe.unit_coding
    lib = os.path.join(hm_tree, "source", "Lib")
    common = os.path.join(os.path.dirname(hm_tree), "hm_common", "c++", "source_common")
    sources = [os.path.join(HERE, "hm_cu_tree_shim.cpp")] + sorted(glob.glob(os.path.join(lib, "TLibCommon", "*.cpp"))) + \
        [os.path.join(lib, "TLibEncoder", name) for name in unit_coding.ENCODER_SOURCES] + sorted(glob.glob(os.path.join(lib, "libmd5", "*.c")))
    flags = ["-O1", "-w", "-ffunction-sections", "-fdata-sections", "-I" + lib, "-I" + common, unit_coding.HM_DEFAULT_TYPES]

    def compile_one(item):
        k, source = item
        obj = os.path.join(build_dir, "%02d_%s.o" % (k, os.path.basename(source)))
        subprocess.check_call((["gcc"] if source.endswith(".c") else ["g++", "-std=c++11"]) + flags + ["-c", source, "-o", obj])
        return obj

    with concurrent.futures.ThreadPoolExecutor(8) as pool:
        objects = list(pool.map(compile_one, enumerate(sources)))
    exe = os.path.join(build_dir, "hm_cu_tree_shim")
    subprocess.check_call(["g++"] + objects + ["-Wl,--gc-sections", "-Wl,--unresolved-symbols=ignore-all", "-o", exe])
    return exe


def main():
    hm_tree = os.path.abspath(sys.argv[1])
    out_dir = sys.argv[3] if len(sys.argv) > 3 else HERE
    with tempfile.TemporaryDirectory() as tmp:
        build_dir = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] else tmp
        text = subprocess.run([build(hm_tree, build_dir)], stdout=subprocess.PIPE, check=True).stdout.decode()
    split = np.full((52, 3, 2), -1, np.int64)
    part = np.full((52, 2), -1, np.int64)
    ctx = np.full((4, 4), 255, np.uint8)
    for line in text.splitlines():
        word, *numbers = line.split()
        numbers = [int(v) for v in numbers]
        if word == "split":
            split[numbers[0], numbers[1], numbers[2]] = numbers[3]
        elif word == "part":
            part[numbers[0], numbers[1]] = numbers[2]
        elif word == "ctx":
            ctx[numbers[0], numbers[1]] = numbers[2]
        else:
            raise AssertionError("an unknown record: %r" % line)
    # conditions on HM's output, not on the code under test
    assert (split > 0).all(), "a split_cu_flag bin was not recorded for every QP, context and value"
    assert (part > 0).all(), "a part_mode bin was not recorded for every QP and value"
    assert (ctx <= 2).all(), "getCtxSplitFlag's truth table is incomplete"
    print("split_cu_flag: %d records, part_mode: %d, contexts:\n%s" % (split.size, part.size, ctx))
    path = os.path.join(out_dir, "hm_cu_tree.npz")
    np.savez_compressed(path, split_bits=split, part_bits=part, split_ctx=ctx)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
