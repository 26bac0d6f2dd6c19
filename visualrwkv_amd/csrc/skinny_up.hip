// C-ABI of the write-wide LoRA product (skinny_up.h): out (M x C) = a (M x R) . w  or  a . w^T.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/visualrwkv_hip.h"
#include <gfx950_prims.h>
#include <host_checks.h>
#include <skinny_up.h>

namespace {

bool rank_ok(int R) { return R == 32 || R == 64 || R == 96 || R == 128 || R == 160 || R == 256; }

// workgroups of four waves a CU holds at once, by the kernel's registers: w fragments R / 2, 32 accumulators, and two narrow tiles of R / 4 each
// where they are registers (74 / 108 / 140 / 204 for R = 32 / 64 / 96 / 160; 138 / 218 for R = 128 / 256, whose tiles are in LDS)
int resident(int R) { return R <= 64 ? 4 : R <= 128 ? 3 : 2; }

// Row groups: one round of the 256 CUs at that residency, a multiple of 8 (the XCD rule of the block id), not more than the row tiles need.
int row_groups(long M, int R, int NW, int NS) {
    const long ntile = (M + skup::TR - 1) / skup::TR;
    long g = (256L * resident(R) * 4 / NW + NS - 1) / NS;
    if (g > ntile) g = ntile;
    return (int)((g + 7) / 8 * 8);
}

template <int R, int NW, bool CXR>
void launch(const skup::Args& a, hipStream_t st) {
    const int NS = a.C / (skup::WC * NW);
    hipLaunchKernelGGL((skup::skinny_up_kernel<R, NW, CXR>), dim3((unsigned)(NS * a.G)), dim3(64 * NW), (size_t)skup::lds_bytes(R, NW), st, a);
}
template <int R>
void launch_r(const skup::Args& a, int NW, bool cxr, hipStream_t st) {
    if (NW == 4) { if (cxr) launch<R, 4, true>(a, st); else launch<R, 4, false>(a, st); }
    else         { if (cxr) launch<R, 2, true>(a, st); else launch<R, 2, false>(a, st); }
}

}  // namespace

extern "C" int vrwkv_skinny_up_bf16(long M, int R, int C, const void* a, const void* w, int w_is_CxR, void* out, void* stream) {
    if (M <= 0 || R <= 0 || C <= 0 || hostchk::any_null(a, w, out)) return VRWKV_EINVAL;
    if (!rank_ok(R) || C % 128 != 0) return VRWKV_ESHAPE;
    if (hostchk::any_misaligned(a, w, out)) return VRWKV_EALIGN;
    const hipStream_t st = (hipStream_t)stream;
    const int NW = C % 256 == 0 ? 4 : 2;                  // a strip of 256 columns; 128 where C is an odd multiple of 128
    const int NS = C / (skup::WC * NW);
    const skup::Args p{M, C, row_groups(M, R, NW, NS), (const uint16_t*)a, (const uint16_t*)w, (uint16_t*)out};
    const bool cxr = w_is_CxR != 0;
    switch (R) {
        case 32: launch_r<32>(p, NW, cxr, st); break;
        case 64: launch_r<64>(p, NW, cxr, st); break;
        case 96: launch_r<96>(p, NW, cxr, st); break;
        case 128: launch_r<128>(p, NW, cxr, st); break;
        case 160: launch_r<160>(p, NW, cxr, st); break;
        default: launch_r<256>(p, NW, cxr, st); break;
    }
    return hostchk::finish_launch();
}
