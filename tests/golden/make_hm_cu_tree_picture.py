"""Generator of tests/golden/hm_cu_tree_picture.npz: TComDataCU::getCtxSplitFlag ACROSS CTU boundaries as HM-16.15 itself answers it,
for tests/test_hm_cu_tree_picture.py.

    python tests/golden/make_hm_cu_tree_picture.py /path/to/hm_16_15_regular [build directory] [output directory]

compiles tests/golden/hm_cu_tree_picture_shim.cpp together with the tree's sources BY PATH the way tests/golden/make_hm_cu_tree.py does
(the same recipe, with this shim) and writes what HM answers.  Only the fixture is kept: recorded numbers, no code.

The world is a 128 x 128 picture of 2 x 2 CTUs in one slice.  Each CTU is given a seeded valid depth map, made here: a quadtree whose
nodes of depths 0 .. 2 split with probability 0.6, written as the depth of each of the 64 minimum-CU cells in z-order.

Layout.  maps uint8 [4][64]: the four maps, CTUs in raster order; seed: the seed that made them; records int64 [44][8], one row per CTU
and node of depths 0 .. 2 that touches the CTU's left or top edge (11 per CTU): CTU, depth, the node's z-order index in its depth,
getCtxSplitFlag, then for the left and for the above side what getPULeft / getPUAbove with their default arguments answered -- state
(0 nothing, 1 shallower, 2 equal, 3 deeper than the node) and whether the CU they returned is ANOTHER CTU (1) or the node's own (0).

The generator FAILS unless every combination of the truth table (nothing, shallower, equal, deeper on each side) occurs across a CTU
boundary at least once: in a record with at least one side answered by another CTU -- or, for (nothing, nothing), which no other CTU
can answer, at the picture's corner.  The seeds 0, 1, ... are tried in turn (at most 200); the states are HM's own answers, not
computed here."""
import glob
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
    """make_hm_cu_tree.build with this generator's shim in the other's place"""
    import concurrent.futures
    unit_coding = recipe.unit_coding
    lib = os.path.join(hm_tree, "source", "Lib")
    common = os.path.join(os.path.dirname(hm_tree), "hm_common", "c++", "source_common")
    sources = [os.path.join(HERE, "hm_cu_tree_picture_shim.cpp")] + sorted(glob.glob(os.path.join(lib, "TLibCommon", "*.cpp"))) + \
        [os.path.join(lib, "TLibEncoder", name) for name in unit_coding.ENCODER_SOURCES] + sorted(glob.glob(os.path.join(lib, "libmd5", "*.c")))
    flags = ["-O1", "-w", "-ffunction-sections", "-fdata-sections", "-I" + lib, "-I" + common, unit_coding.HM_DEFAULT_TYPES]

    def compile_one(item):
        k, source = item
        obj = os.path.join(build_dir, "%02d_%s.o" % (k, os.path.basename(source)))
        subprocess.check_call((["gcc"] if source.endswith(".c") else ["g++", "-std=c++11"]) + flags + ["-c", source, "-o", obj])
        return obj

    with concurrent.futures.ThreadPoolExecutor(8) as pool:
        objects = list(pool.map(compile_one, enumerate(sources)))
    exe = os.path.join(build_dir, "hm_cu_tree_picture_shim")
    subprocess.check_call(["g++"] + objects + ["-Wl,--gc-sections", "-Wl,--unresolved-symbols=ignore-all", "-o", exe])
    return exe


def seeded_map(rng):
    """The depth of the 64 minimum-CU cells of one CTU in z-order: node i of depth d covers the cells [i, i + 1) * 4^(3 - d)"""
    cells = np.zeros(64, np.uint8)

    def fill(depth, first):
        count = 64 >> (2 * depth)
        if depth < 3 and rng.random() < 0.6:
            for k in range(4):
                fill(depth + 1, first + k * (count // 4))
        else:
            cells[first:first + count] = depth

    fill(0, 0)
    return cells


def covered(records):
    table = np.zeros((4, 4), bool)
    for ctu, depth, node, ctx, left, left_other, above, above_other in records:
        if left_other or above_other or (left == 0 and above == 0):
            table[left, above] = True
    return table


def main():
    hm_tree = os.path.abspath(sys.argv[1])
    out_dir = sys.argv[3] if len(sys.argv) > 3 else HERE
    with tempfile.TemporaryDirectory() as tmp:
        build_dir = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] else tmp
        exe = build(hm_tree, build_dir)
        chosen = None
        for seed in range(200):
            rng = np.random.default_rng(seed)
            maps = np.stack([seeded_map(rng) for _ in range(4)])
            path = os.path.join(tmp, "maps.txt")
            np.savetxt(path, maps, fmt="%d")
            text = subprocess.run([exe, path], stdout=subprocess.PIPE, check=True).stdout.decode()
            records = []
            for line in text.splitlines():
                word, *numbers = line.split()
                assert word == "ctx", "an unknown record: %r" % line
                records.append([int(v) for v in numbers])
            records = np.array(records, np.int64)
            # conditions on HM's output, not on the code under test
            assert records.shape == (44, 8), "not 11 records per CTU"
            table = covered(records)
            print("seed %d: %d of 16 combinations across a CTU boundary" % (seed, int(table.sum())))
            if table.all():
                chosen = (seed, maps, records)
                break
    assert chosen is not None, "no seed of 0 .. 199 gives every combination of the truth table across a CTU boundary"
    seed, maps, records = chosen
    assert (records[:, 3] <= 2).all()
    print("maps (CTU by CTU, z-order):\n%s\nrecords:\n%s" % (maps, records))
    path = os.path.join(out_dir, "hm_cu_tree_picture.npz")
    np.savez_compressed(path, maps=maps, seed=np.int64(seed), records=records)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
