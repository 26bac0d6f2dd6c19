// csrc/skinny_up.hip -- the kernel of skinny_up.h AND its C entry point with the launch logic (strip width, row groups, the argument checks) --
// compiled for the host lockstep emulator: the same vrwkv_skinny_up_bf16 symbol as the product library, computed on the CPU.  TEST INFRASTRUCTURE ONLY.
#include <hip/hip_runtime.h>
#include <gfx950_prims.h>
#include "../../visualrwkv_amd/csrc/skinny_up.hip"

// The same launch with a caller-chosen number of row groups G (a multiple of 8): the entry point gives every row tile a workgroup of its own until M
// passes 8 192 rows or more, which the emulator walks in minutes; with G = 8 a few hundred rows make a workgroup walk several tiles (the prefetched
// narrow tile, the reuse of the wave's LDS image).
extern "C" int emu_skinny_up_groups(long M, int R, int C, int G, const void* a, const void* w, int w_is_CxR, void* out) {
    if (M <= 0 || R <= 0 || C <= 0 || G <= 0 || !a || !w || !out) return VRWKV_EINVAL;
    if (!rank_ok(R) || C % 128 != 0 || G % 8 != 0) return VRWKV_ESHAPE;
    const int NW = C % 256 == 0 ? 4 : 2;
    const skup::Args p{M, C, G, (const uint16_t*)a, (const uint16_t*)w, (uint16_t*)out};
    const bool cxr = w_is_CxR != 0;
    switch (R) {
        case 32: launch_r<32>(p, NW, cxr, nullptr); break;
        case 64: launch_r<64>(p, NW, cxr, nullptr); break;
        case 96: launch_r<96>(p, NW, cxr, nullptr); break;
        case 128: launch_r<128>(p, NW, cxr, nullptr); break;
        case 160: launch_r<160>(p, NW, cxr, nullptr); break;
        default: launch_r<256>(p, NW, cxr, nullptr); break;
    }
    return VRWKV_OK;
}
