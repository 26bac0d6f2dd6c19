// Device helpers shared by the one-token decode kernels (gemv_decode.hip, decode_fused.hip, decode6_fused.hip, wkv7_step.hip, wkv6_step.hip):
// 8 x bf16 <-> 8 x fp32 through 16-byte registers, the 64 x 64 state tile through LDS, the GroupNorm over a head.
// Device code only (the host side of these files is host_checks.h); the emulator builds (tests/emu) include it with the translation units that use it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <gfx950_prims.h>

namespace decode {

// 16-byte register pieces as the compiler's NATIVE vector type: private arrays of HIP's uint4 (a struct of unions) are not
// promoted to registers and ended up in scratch memory (32 B/lane in the LayerNorm prologues of gemv_decode.hip and decode_fused.hip).
typedef uint32_t vrwkv_u4 __attribute__((ext_vector_type(4)));

DEVFN float rb(float x) { return __uint_as_float(f32_to_bf16_bits(x) << 16); }     // round to bf16, keep as fp32

DEVFN void unpack8(const vrwkv_u4& u, float* f) {
    f[0] = bf16_lo(u.x); f[1] = bf16_hi(u.x); f[2] = bf16_lo(u.y); f[3] = bf16_hi(u.y);
    f[4] = bf16_lo(u.z); f[5] = bf16_hi(u.z); f[6] = bf16_lo(u.w); f[7] = bf16_hi(u.w);
}
DEVFN vrwkv_u4 pack8(const float* f) {
    return vrwkv_u4{pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]), pack_bf16x2(f[4], f[5]), pack_bf16x2(f[6], f[7])};
}
DEVFN vrwkv_u4 ld16(const uint16_t* p) { return *reinterpret_cast<const vrwkv_u4*>(p); }

// The 64 x 64 fp32 state tile of one head, staged through S[64][65] in LDS (row stride padded so that a per-lane row or column walk is
// bank-conflict free) with 16-byte coalesced global accesses: 1024 float4, vector e = row e >> 4, columns (e & 15) * 4 .. + 3.
// The loops over e stay in the kernels: the one-wave step kernels walk e = lane, lane + 64, .. in a rolled loop, the 256-thread head kernels
// hold their four vectors in registers from before their other global loads until those are issued too (a helper that took the register
// array or hid the loop changed the kernels' schedules and register counts).
constexpr int STATE_VECS = 1024;

DEVFN void state_put(float (&S)[64][65], int e, const float4& x) {
    const int r = e >> 4, c = (e & 15) * 4;
    S[r][c] = x.x; S[r][c + 1] = x.y; S[r][c + 2] = x.z; S[r][c + 3] = x.w;
}
DEVFN float4 state_get(const float (&S)[64][65], int e) {
    const int r = e >> 4, c = (e & 15) * 4;
    return make_float4(S[r][c], S[r][c + 1], S[r][c + 2], S[r][c + 3]);
}
// GroupNorm over the 64 channels of a head, one channel per lane of the wave: returns y - mean, sets rstd (biased variance around the mean).
DEVFN float groupnorm64(float y, float eps, float& rstd) {
    const float mean = group_sum<6>(y) * (1.f / 64.f);
    const float dlt = y - mean;
    rstd = fast_rsqrt(group_sum<6>(dlt * dlt) * (1.f / 64.f) + eps);
    return dlt;
}

}  // namespace decode
