// WKV6 single-token step with carried state (stateful RWKV-6 generation).
//
// The reference has no stateful RWKV-6 path: its generate re-runs the whole text pass for every new token.  Same recurrence as
// kernel_forward of cuda/wkv6_cuda.cu for T = 1 (the time-mix of VisualRWKV-v6/v6.0/src/model.py:92-226; the carried state of
// v6.xx/src/model.py:137-144), with the per-head state S (fp32, [key i][value j]: the layout of vrwkv_wkv6_forward_state_bf16) read and
// written in place:
//     y[j] = sum_i r[i] (u[i] k[i] v[j] + S[i][j]) ;   S[i][j] = S[i][j] w[i] + k[i] v[j]           w = exp(-exp(w_raw))
// One wave per (b,h): lane j owns value column j.  The 16 KB state tile is staged through LDS (decode_common.h); the five 128-byte
// vectors come in as one 16-byte load per lane.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/visualrwkv_hip.h"
#include <gfx950_prims.h>
#include "decode_common.h"
#include "host_checks.h"

namespace {

using namespace decode;

constexpr int W6_MAX_B = 4;
constexpr int W6_MAX_H = 128;                  // C = 64 H <= 8192

__global__ __launch_bounds__(64) void wkv6_step_kernel(int H, const uint16_t* __restrict__ r_, const uint16_t* __restrict__ k_,
                                                       const uint16_t* __restrict__ v_, const uint16_t* __restrict__ w_,
                                                       const uint16_t* __restrict__ u_, float* __restrict__ state,
                                                       uint16_t* __restrict__ y_) {
    __shared__ float S[64][65];
    __shared__ float vec[5][64];                   // r k decay u v
    __shared__ __attribute__((aligned(16))) uint16_t yb[64];
    const int bh = blockIdx.x, l = threadIdx.x;
    const size_t vb = (size_t)bh * 64;
    float* sp = state + (size_t)bh * 64 * 64;
    if (l < 40) {                                  // lanes 8 m .. 8 m + 7: vector m, 8 elements each
        const int m = l >> 3, c = (l & 7) * 8;
        const uint16_t* src = m == 0 ? r_ + vb : m == 1 ? k_ + vb : m == 2 ? w_ + vb : m == 3 ? u_ + (size_t)(bh % H) * 64 : v_ + vb;
        float* d = &vec[m][c];
        unpack8(ld16(src + c), d);
        if (m == 2)
#pragma unroll
            for (int e = 0; e < 8; ++e) d[e] = fast_exp(-fast_exp(d[e]));
    }
    for (int e = l; e < STATE_VECS; e += 64) state_put(S, e, reinterpret_cast<const float4*>(sp)[e]);
    __syncthreads();
    const float vj = vec[4][l];
    float y = 0.f;
#pragma unroll 8
    for (int i = 0; i < 64; ++i) {
        const float s = S[i][l], kv = vec[1][i] * vj;
        y = fmaf(vec[0][i], fmaf(vec[3][i], kv, s), y);
        S[i][l] = fmaf(s, vec[2][i], kv);
    }
    yb[l] = (uint16_t)f32_to_bf16_bits(y);
    __syncthreads();
    if (l < 8) *reinterpret_cast<vrwkv_u4*>(y_ + vb + l * 8) = *reinterpret_cast<const vrwkv_u4*>(&yb[l * 8]);
    for (int e = l; e < STATE_VECS; e += 64) reinterpret_cast<float4*>(sp)[e] = state_get(S, e);
}

}  // namespace

extern "C" int vrwkv_wkv6_step_bf16(int B, int H, const void* r, const void* k, const void* v, const void* w_raw, const void* u,
                                    float* state, void* y, void* stream) {
    if (B <= 0 || B > W6_MAX_B || H <= 0 || hostchk::any_null(r, k, v, w_raw, u, state, y)) return VRWKV_EINVAL;
    if (H > W6_MAX_H) return VRWKV_ESHAPE;
    if (hostchk::any_misaligned(r, k, v, w_raw, u, state, y)) return VRWKV_EALIGN;
    hipLaunchKernelGGL(wkv6_step_kernel, dim3((unsigned)(B * H)), dim3(64), 0, (hipStream_t)stream, H, (const uint16_t*)r,
                       (const uint16_t*)k, (const uint16_t*)v, (const uint16_t*)w_raw, (const uint16_t*)u, state, (uint16_t*)y);
    return hostchk::finish_launch();
}
