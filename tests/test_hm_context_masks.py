"""Context availability (include/pnn_hip.h, "context availability"): pnn_hm_context_masks_host and
intraprediction.hm_context_masks against what HM-16.15's own isAboveRightAvailable / isBelowLeftAvailable answered
(tests/golden/hm_context_masks.npz, made by tests/golden/make_hm_context_masks.py), against a brute-force restatement of the header's
table on other grids, and against known answers; every refusal; and tests/sanitize_context_masks.cpp, a stand-alone program over the host
entry under AddressSanitizer + UBSan (built and run the way tests/test_cu_tree_sanitizer.py builds and runs its program)."""
import os
import subprocess

import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import _lib, intraprediction

HERE = os.path.dirname(os.path.abspath(__file__))
WIDTHS = (4, 8, 16, 32, 64)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "hm_context_masks.npz"))


def z_of(x, y):
    return sum(((x >> j) & 1) << (2 * j) | ((y >> j) & 1) << (2 * j + 1) for j in range(4))


def restated(w, rows, cols):
    """The header's table, block by block, with nothing shared with the library: (mask_w, mask_h) in (CTU raster, z-order) order."""
    n, side = w // 4, 64 // w
    mask_w, mask_h = [], []
    for r in range(rows):
        for c in range(cols):
            blocks = sorted((z_of(bx, by), bx * n, by * n) for bx in range(side) for by in range(side))
            for _, x, y in blocks:
                if x + n < 16 and y > 0:
                    above_right = z_of(x + n, y - 1) < z_of(x + n - 1, y)
                elif x + n < 16:
                    above_right = r > 0
                elif y > 0:
                    above_right = False
                else:
                    above_right = r > 0 and c + 1 < cols
                if y + n == 16:
                    below_left = False
                elif x > 0:
                    below_left = z_of(x - 1, y + n) < z_of(x, y + n - 1)
                else:
                    below_left = c > 0
                mask_w.append(0 if above_right else w)
                mask_h.append(0 if below_left else w)
    return np.array(mask_w, np.uint8), np.array(mask_h, np.uint8)


def host_masks(w, rows, cols):
    count = rows * cols * (64 // w) ** 2
    mask_w, mask_h = np.full(count, 7, np.uint8), np.full(count, 7, np.uint8)
    assert _lib.lib().pnn_hm_context_masks_host(w, rows, cols, mask_w.ctypes.data, mask_h.ctypes.data) == 0
    return mask_w, mask_h


def test_fixture_is_complete(golden):
    records = golden["records"]
    assert records.shape == (4 * 341, 9)
    seen = {(int(r[0]), int(r[1]), int(r[2])) for r in records}
    assert seen == {(ctu, w, z) for ctu in range(4) for w in WIDTHS for z in range((64 // w) ** 2)}
    for flags_name, column in (("flags_above_right", 7), ("flags_below_left", 8)):
        flags = golden[flags_name]
        assert flags.shape == (4 * 341, 16)
        for record, row in zip(records, flags):
            n = int(record[1]) // 4
            assert (row[:n] == record[column]).all() and (row[n:] == -1).all()         # all or nothing: HM's answer
            assert record[column - 2] == n * record[column]                            # the return value counts the flags
    for record in records:                                                             # (x, y) is the z-order's
        n = int(record[1]) // 4
        assert z_of(int(record[3]) // n, int(record[4]) // n) == record[2]


@pytest.mark.parametrize("w", WIDTHS)
def test_equals_hm_on_the_2x2_grid(golden, w):
    records = golden["records"]
    per_ctu = (64 // w) ** 2
    want_w, want_h = np.empty(4 * per_ctu, np.uint8), np.empty(4 * per_ctu, np.uint8)
    for ctu, width, z, _, _, _, _, above_right, below_left in records[records[:, 1] == w]:
        want_w[ctu * per_ctu + z] = 0 if above_right else w
        want_h[ctu * per_ctu + z] = 0 if below_left else w
    for got_w, got_h in (host_masks(w, 2, 2), intraprediction.hm_context_masks(w, 2, 2)):
        assert got_w.dtype == np.uint8 and got_h.dtype == np.uint8
        assert np.array_equal(got_w, want_w) and np.array_equal(got_h, want_h)
    assert all(np.array_equal(a, b) for a, b in zip(restated(w, 2, 2), (want_w, want_h)))      # the restatement itself is HM's answer here


@pytest.mark.parametrize("grid", [(1, 1), (1, 3), (3, 1), (2, 3)])
@pytest.mark.parametrize("w", WIDTHS)
def test_equals_the_restatement_on_other_grids(w, grid):
    want = restated(w, *grid)
    for got in (host_masks(w, *grid), intraprediction.hm_context_masks(w, *grid)):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_order_is_that_of_ctu_block_positions():
    """The block at index i is the one ctu_block_positions puts there: its unit (x, y) decides the answer inside a CTU."""
    for w in WIDTHS:
        rows, cols = intraprediction.ctu_block_positions(w, *intraprediction.ctu_grid(64, 64, 1, 1))
        x, y = (cols + w - 64) // 4, (rows + w - 64) // 4
        mask_w, mask_h = intraprediction.hm_context_masks(w, 1, 1)
        n = w // 4
        for i in range(rows.size):
            inside = x[i] + n < 16 and y[i] > 0
            if inside:
                assert (mask_w[i] == 0) == (z_of(x[i] + n, y[i] - 1) < z_of(x[i] + n - 1, y[i]))
            if x[i] > 0 and y[i] + n < 16:
                assert (mask_h[i] == 0) == (z_of(x[i] - 1, y[i] + n) < z_of(x[i], y[i] + n - 1))


@pytest.mark.parametrize("grid", [(1, 1), (2, 2), (2, 3), (3, 1)])
def test_known_answers(grid):
    rows, cols = grid
    mask_w, mask_h = intraprediction.hm_context_masks(64, rows, cols)
    assert (mask_h == 64).all()
    want = np.array([0 if r > 0 and c + 1 < cols else 64 for r in range(rows) for c in range(cols)], np.uint8)
    assert np.array_equal(mask_w, want)
    for w in WIDTHS:
        per_ctu = (64 // w) ** 2
        mask_w, mask_h = (m.reshape(rows * cols, per_ctu) for m in intraprediction.hm_context_masks(w, rows, cols))
        for r in range(rows):
            for c in range(cols):
                ctu = r * cols + c
                if r > 0 and w < 64:
                    assert mask_w[ctu, 0] == 0                                          # the first block under a coded CTU row
                if w < 64:                                                              # (at 64 the last block is the first: the answer above)
                    assert mask_w[ctu, -1] == w and mask_h[ctu, -1] == w                # the z-order's last block has neither


@pytest.mark.parametrize("w", (4, 8, 16, 32))
def test_floor_all_four_combinations_occur(w):
    """From the restatement alone: the 2 x 2 grid exercises every combination of the two masks at every width below 64."""
    mask_w, mask_h = restated(w, 2, 2)
    assert {(int(a), int(b)) for a, b in zip(mask_w, mask_h)} == {(0, 0), (0, w), (w, 0), (w, w)}


def test_refusals():
    L = _lib.lib()
    a, b = np.full(256, 7, np.uint8), np.full(256, 7, np.uint8)
    for w in (0, -4, 2, 12, 65, 128):
        assert L.pnn_hm_context_masks_host(w, 1, 1, a.ctypes.data, b.ctypes.data) != 0
        with pytest.raises(ValueError):
            intraprediction.hm_context_masks(w, 1, 1)
    for grid in ((0, 1), (1, 0), (-1, 2), (2, -1)):
        assert L.pnn_hm_context_masks_host(4, grid[0], grid[1], a.ctypes.data, b.ctypes.data) != 0
        with pytest.raises(ValueError):
            intraprediction.hm_context_masks(4, *grid)
    for bad in (1.5, True, None):
        with pytest.raises(ValueError):
            intraprediction.hm_context_masks(4, bad, 1)
    assert L.pnn_hm_context_masks_host(4, 1 << 16, 1 << 16, a.ctypes.data, b.ctypes.data) != 0
    assert L.pnn_hm_context_masks_host(4, 1, 1, None, b.ctypes.data) != 0
    assert L.pnn_hm_context_masks_host(4, 1, 1, a.ctypes.data, None) != 0
    assert (a == 7).all() and (b == 7).all()                                            # nothing written by a refused call


def test_sanitizer_program(tmp_path):
    root = os.path.dirname(HERE)
    csrc = os.path.join(root, "context_adaptive_neural_network_based_prediction_amd", "csrc")
    exe = str(tmp_path / "sanitize_context_masks")
    r = subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1", "-std=c++17",
                        "-Wall", "-Wextra", "-I" + os.path.join(root, "include"), os.path.join(HERE, "sanitize_context_masks.cpp"),
                        os.path.join(csrc, "pnn_context_masks.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "sanitize_context_masks: ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
