// The carry instantiations of the token-shift kernels of csrc/ln_kernels.h (one segment of a longer row: y_prev / y_last forward,
// y_prev / dy_last / dy_prev backward) under the host lockstep emulator.  TEST INFRASTRUCTURE ONLY.  The third carry entry,
// vrwkv_mix_bwd_ln_carry_bf16, comes in whole through emu_tmix.cpp.
#include <gfx950_prims.h>
#include <vector>
namespace {                 // emu_ln.cpp holds the external definitions of this header's non-template kernels
#include <ln_kernels.h>
}

using namespace vln;

static int threads_for_carry(int C) { return (C / 8 + 63) / 64 * 64; }

extern "C" int emu_ln_mix_fwd_carry(long ntok, int T, int C, float eps, int M, const void* x, const void* delta, const void* w, const void* b,
                                    const void* const* mu, void* xn, void* const* out, float* mean, float* rstd, const void* y_prev, void* y_last,
                                    int grid) {
    LmPtrs pm{}; LmOuts po{};
    for (int j = 0; j < M; ++j) { pm.p[j] = (const uint16_t*)mu[j]; po.p[j] = (uint16_t*)out[j]; }
    const dim3 g((unsigned)grid), blk((unsigned)threads_for_carry(C));
    if (M == 1) emu::launch(g, blk, [&] { ln_mix_fwd_kernel<1, false, true>(ntok, T, C, eps, (const uint16_t*)x, (const uint16_t*)delta, (const uint16_t*)w, (const uint16_t*)b, (uint16_t*)xn, mean, rstd, pm, po, nullptr, (const uint16_t*)y_prev, (uint16_t*)y_last); });
    else if (M == 6) emu::launch(g, blk, [&] { ln_mix_fwd_kernel<6, false, true>(ntok, T, C, eps, (const uint16_t*)x, (const uint16_t*)delta, (const uint16_t*)w, (const uint16_t*)b, (uint16_t*)xn, mean, rstd, pm, po, nullptr, (const uint16_t*)y_prev, (uint16_t*)y_last); });
    else return -1;
    return 0;
}

extern "C" int emu_ln_mix_bwd1_carry(long ntok, int T, int C, const void* xn, const float* mean, const float* rstd, const void* w, const void* b,
                                     const void* mu, const void* dout, const void* dres, const void* y_prev, const float* dy_last, float* dy_prev,
                                     void* dx, float* dwb, float* dmu, int grid) {
    LmPtrs pm{}, pd{};
    pm.p[0] = (const uint16_t*)mu; pd.p[0] = (const uint16_t*)dout;
    std::vector<float> part_ln((size_t)grid * 2 * C), part_mu((size_t)grid * C);
    float* pl = part_ln.data(); float* pmu = part_mu.data();
    emu::launch(dim3((unsigned)grid), dim3((unsigned)threads_for_carry(C)), [&] {
        ln_mix_bwd_kernel<1, false, 256, false, true>(ntok, T, C, (const uint16_t*)xn, mean, rstd, (const uint16_t*)w, (const uint16_t*)b, pm, pd,
                                                      (const uint16_t*)nullptr, (const uint16_t*)dres, (uint16_t*)dx, pl, pmu, nullptr,
                                                      (const uint16_t*)y_prev, dy_last, dy_prev); });
    emu::launch(dim3((unsigned)(2L * C / 16)), dim3(256), [&] { ln_colsum_kernel(grid, 2L * C, pl, dwb); });
    emu::launch(dim3((unsigned)(C / 16)), dim3(256), [&] { ln_colsum_kernel(grid, (long)C, pmu, dmu); });
    return 0;
}
