// Stand-alone program over pnn_hm_context_masks_host (include/pnn_hip.h, "context availability"), built under AddressSanitizer + UBSan
// (tests/test_hm_context_masks.py compiles it together with csrc/pnn_context_masks.cpp): every width on grids of 1 x 1, 1 x 3, 3 x 1,
// 2 x 3 and 5 x 4 CTUs into buffers of EXACTLY the documented size (a write past them is a heap overflow the sanitizer reports), every
// value 0 or the width, and every refusal with the outputs untouched.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pnn_hip.h"

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); failures++; } \
    } while (0)

int main()
{
    const int widths[5] = {4, 8, 16, 32, 64};
    const int grids[5][2] = {{1, 1}, {1, 3}, {3, 1}, {2, 3}, {5, 4}};
    for (int w : widths)
        for (const auto& g : grids) {
            const size_t count = (size_t)g[0] * g[1] * (64 / w) * (64 / w);
            std::vector<uint8_t> mw(count, 7), mh(count, 7);
            EXPECT(pnn_hm_context_masks_host(w, g[0], g[1], mw.data(), mh.data()) == PNN_OK);
            for (size_t i = 0; i < count; i++) EXPECT((mw[i] == 0 || mw[i] == w) && (mh[i] == 0 || mh[i] == w));
            // the z-order's last block of every CTU has neither portion (at width 64 it is the CTU's only block, which may have the first)
            const size_t per_ctu = count / ((size_t)g[0] * g[1]);
            for (size_t ctu = 0; w < 64 && ctu < (size_t)g[0] * g[1]; ctu++)
                EXPECT(mw[ctu * per_ctu + per_ctu - 1] == w && mh[ctu * per_ctu + per_ctu - 1] == w);
        }
    uint8_t a[256], b[256];
    for (int i = 0; i < 256; i++) a[i] = b[i] = 7;
    const int bad_widths[6] = {0, -4, 2, 12, 128, 65};
    for (int w : bad_widths) EXPECT(pnn_hm_context_masks_host(w, 1, 1, a, b) == PNN_E_ARG);
    EXPECT(pnn_hm_context_masks_host(4, 0, 1, a, b) == PNN_E_ARG);
    EXPECT(pnn_hm_context_masks_host(4, 1, 0, a, b) == PNN_E_ARG);
    EXPECT(pnn_hm_context_masks_host(4, -1, 2, a, b) == PNN_E_ARG);
    EXPECT(pnn_hm_context_masks_host(4, 1 << 16, 1 << 16, a, b) == PNN_E_ARG);
    EXPECT(pnn_hm_context_masks_host(4, 1, 1, nullptr, b) == PNN_E_ARG);
    EXPECT(pnn_hm_context_masks_host(4, 1, 1, a, nullptr) == PNN_E_ARG);
    for (int i = 0; i < 256; i++) EXPECT(a[i] == 7 && b[i] == 7);
    if (failures) { printf("sanitize_context_masks: %d failures\n", failures); return 1; }
    printf("sanitize_context_masks: ok\n");
    return 0;
}
