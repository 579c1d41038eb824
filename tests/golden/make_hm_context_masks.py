"""Generator of tests/golden/hm_context_masks.npz: which above-right and below-left neighbours a block has, as HM-16.15 itself answers
it (isAboveRightAvailable / isBelowLeftAvailable of TComPattern.cpp), for tests/test_hm_context_masks.py.

    python tests/golden/make_hm_context_masks.py /path/to/hm_16_15_regular [build directory] [output directory]

compiles tests/golden/hm_context_masks_shim.cpp together with the tree's sources BY PATH (tests/golden/hm_shim_recipe.py: the recipe of
tests/golden/make_hm_cu_tree_picture.py, written once with the shim as its argument) and writes what HM answers.  Only the fixture is kept: recorded numbers, no code.

The world is a 128 x 128 picture of 2 x 2 CTUs in one slice and one tile, constrained intra prediction off.  For every CTU, every one of
the five widths and every aligned block the shim calls the two functions with the block's LT / RT / LB partitions, as
TComPrediction::initIntraPatternChType does.

Layout.  records int64 [4 * 341][9], one row per (CTU, width, block): CTU (raster), width, the block's z-order index among the CTU's
blocks of its width, its first unit (x, y) in the CTU, the return value of isAboveRightAvailable, that of isBelowLeftAvailable, then
the two answers as ONE flag each (1 available, 0 not); flags_above_right, flags_below_left int8 [4 * 341][16]: the width / 4 flags each
function wrote (left to right, top to bottom), -1 behind them.  The generator FAILS unless, for every block, the flags each function
wrote are all equal and agree with its return value (0 or width / 4): the all-or-nothing claim of include/pnn_hip.h, "context
availability", as HM's own answer.  It also FAILS unless every block of every CTU and width is recorded exactly once."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
import hm_shim_recipe  # noqa: E402

WIDTHS = (4, 8, 16, 32, 64)


def main():
    hm_tree = os.path.abspath(sys.argv[1])
    out_dir = sys.argv[3] if len(sys.argv) > 3 else HERE
    with tempfile.TemporaryDirectory() as tmp:
        build_dir = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] else tmp
        exe = hm_shim_recipe.build(hm_tree, build_dir, "hm_context_masks_shim")
        text = subprocess.run([exe], stdout=subprocess.PIPE, check=True).stdout.decode()
    records, seen, all_ar, all_bl = [], set(), [], []
    for line in text.splitlines():
        word, *numbers = line.split()
        assert word == "blk", "an unknown record: %r" % line
        numbers = [int(v) for v in numbers]
        ctu, width, z, x, y, count_ar, count_bl = numbers[:7]
        n = width // 4
        flags_ar, flags_bl = numbers[7:7 + n], numbers[7 + n:7 + 2 * n]
        assert len(numbers) == 7 + 2 * n, "a record of the wrong length: %r" % line
        # conditions on HM's output, not on the code under test: all or nothing, and the counts agree with the flags
        assert len(set(flags_ar)) == 1 and count_ar == sum(flags_ar), "the above-right flags of %r are not all equal" % line
        assert len(set(flags_bl)) == 1 and count_bl == sum(flags_bl), "the below-left flags of %r are not all equal" % line
        assert (ctu, width, z) not in seen, "a block recorded twice: %r" % line
        seen.add((ctu, width, z))
        records.append([ctu, width, z, x, y, count_ar, count_bl, flags_ar[0], flags_bl[0]])
        all_ar.append(flags_ar + [-1] * (16 - n))
        all_bl.append(flags_bl + [-1] * (16 - n))
    wanted = {(ctu, w, z) for ctu in range(4) for w in WIDTHS for z in range((64 // w) ** 2)}
    assert seen == wanted, "%d of %d blocks recorded" % (len(seen & wanted), len(wanted))
    records = np.array(records, np.int64)
    path = os.path.join(out_dir, "hm_context_masks.npz")
    np.savez_compressed(path, records=records, flags_above_right=np.array(all_ar, np.int8), flags_below_left=np.array(all_bl, np.int8))
    print("%s: %d records, %d bytes" % (path, len(records), os.path.getsize(path)))


if __name__ == "__main__":
    main()
