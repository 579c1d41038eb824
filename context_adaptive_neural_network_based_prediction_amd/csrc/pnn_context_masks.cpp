// Context availability (no HIP in this file; include/pnn_hip.h, "context availability"): per aligned block of a grid
// of whole CTUs, whether HM-16.15 holds the block's above-right and below-left neighbours when it predicts the block, written as the
// masks of the picture entries.  The definition is the header's text; tests/test_hm_context_masks.py pins this file to what HM's own
// isAboveRightAvailable / isBelowLeftAvailable answer (tests/golden/hm_context_masks.npz) and to a restatement of the header's table.
#include "../../include/pnn_hip.h"

#include <cstdint>
#include <cstdio>

namespace {

constexpr int kCtu = 64, kUnits = 16;                      // a CTU in samples and in 4 x 4 units

// z-order index of unit (x, y) of a CTU: bit 2 j is bit j of x, bit 2 j + 1 bit j of y
int z_of(int x, int y)
{
    int z = 0;
    for (int j = 0; j < 4; j++) z |= ((x >> j) & 1) << (2 * j) | ((y >> j) & 1) << (2 * j + 1);
    return z;
}

// the block of n units at unit (x, y) of the CTU at (r, c) of a grid with `cols` CTU columns
bool above_right_available(int x, int y, int n, int r, int c, int cols)
{
    if (x + n < kUnits) return y > 0 ? z_of(x + n, y - 1) < z_of(x + n - 1, y) : r > 0;
    return y == 0 && r > 0 && c + 1 < cols;
}
bool below_left_available(int x, int y, int n, int c)
{
    if (y + n == kUnits) return false;
    return x > 0 ? z_of(x - 1, y + n) < z_of(x, y + n - 1) : c > 0;
}

}  // namespace

extern "C" int pnn_hm_context_masks_host(int width, int ctu_rows, int ctu_cols, uint8_t* mask_w, uint8_t* mask_h)
{
    const char* refusal = nullptr;
    if (width != 4 && width != 8 && width != 16 && width != 32 && width != 64) refusal = "the width is not 4, 8, 16, 32 or 64";
    else if (ctu_rows < 1 || ctu_cols < 1) refusal = "ctu_rows or ctu_cols is below 1";
    else if ((long long)ctu_rows * ctu_cols * ((kCtu / width) * (kCtu / width)) > 0x7fffffffLL) refusal = "the blocks of the grid do not fit an int";
    else if (!mask_w || !mask_h) refusal = "an output is NULL";
    if (refusal) { fprintf(stderr, "pnn_hm_context_masks_host: %s.\n", refusal); return PNN_E_ARG; }
    const int side = kCtu / width, n = width / 4;
    size_t at = 0;
    for (int r = 0; r < ctu_rows; r++)
        for (int c = 0; c < ctu_cols; c++)
            for (int i = 0; i < side * side; i++, at++) {
                int bx = 0, by = 0;                          // the block's place in the CTU from its z-order index
                for (int j = 0; j < 4; j++) { bx |= ((i >> (2 * j)) & 1) << j; by |= ((i >> (2 * j + 1)) & 1) << j; }
                const int x = bx * n, y = by * n;
                mask_w[at] = above_right_available(x, y, n, r, c, ctu_cols) ? 0 : (uint8_t)width;
                mask_h[at] = below_left_available(x, y, n, c) ? 0 : (uint8_t)width;
            }
    return PNN_OK;
}
