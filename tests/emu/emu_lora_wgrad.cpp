// csrc/lora_wgrad.hip -- the C entry points of both weight-gradient kernels with their launch logic (splits, big_splits, the D / 16 switch,
// the ws contracts, the reduce grid cap, the argument checks) -- compiled for the host lockstep emulator: the same vrwkv_wgrad_* symbols as
// the product library, computed on the CPU.  TEST INFRASTRUCTURE ONLY.
#include <hip/hip_runtime.h>
#include <gfx950_prims.h>
namespace {                 // emu_wkv7.cpp holds the external definitions of these headers' non-template kernels
#include <lora_wgrad.h>
#include <wgrad_big.h>
}
#include "../../visualrwkv_amd/csrc/lora_wgrad.hip"

// The skinny kernel with a caller-chosen number of M-slices S (1 <= S <= steps): slices of several steps need Nw M of a few million elements
// through splits(), which the emulator walks in tens of seconds; here they cost a 128-column launch.  Same D -> ND switch as the entry point
// above (D = 256: two column groups of <8>), then reduce_kernel.  part: S Nw D floats.
extern "C" int emu_wgrad_skinny_slices(long M, int Nw, int D, int S, const void* wide, const void* narrow, float* part, void* out, int transposed) {
    if (M <= 0 || !wide || !narrow || !out || !part) return VRWKV_EINVAL;
    if (Nw <= 0 || Nw % lwg::CT != 0 || !supported_d(D) || S < 1 || S > (M + lwg::KS - 1) / lwg::KS) return VRWKV_ESHAPE;
    const lwg::Args a{M, Nw, D, (const uint16_t*)wide, (const uint16_t*)narrow, part};
    switch (D / 16) {
        case 2: launch<2>(a, S, nullptr); break;
        case 4: launch<4>(a, S, nullptr); break;
        case 6: launch<6>(a, S, nullptr); break;
        case 8: launch<8>(a, S, nullptr); break;
        case 10: launch<10>(a, S, nullptr); break;
        default: launch<8>(a, S, nullptr); break;
    }
    const long n = (long)Nw * D;
    hipLaunchKernelGGL(lwg::reduce_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, nullptr, part, S, Nw, D, transposed, (uint16_t*)out);
    return VRWKV_OK;
}
