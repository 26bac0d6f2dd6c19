// WKV7 single-token step with carried state (stateful generation).
//
// The reference has no stateful RWKV-7 path: VisualRWKV.generate re-runs the full training forward for every new
// token (VisualRWKV-v7/v7.00/src/model.py:513-529).  Same recurrence as forward_kernel (cuda/wkv7_cuda.cu:17-42)
// for T = 1, with the per-head state S (fp32, [i][j], i = value row, j = key column) read and written in place:
//     sa = S z ;  S = S diag(w) + sa a^T + v k^T ;  y = S q          w = exp(-exp(w_raw))
// One wave per (b,h): lane i owns row i.  The 16 KB state tile is staged through LDS (decode_common.h).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/visualrwkv_hip.h"
#include <gfx950_prims.h>
#include "decode_common.h"
#include "host_checks.h"

namespace {

using namespace decode;

__global__ __launch_bounds__(64) void wkv7_step_kernel(int H, const uint16_t* __restrict__ w_, const uint16_t* __restrict__ q_,
                                                       const uint16_t* __restrict__ k_, const uint16_t* __restrict__ v_,
                                                       const uint16_t* __restrict__ z_, const uint16_t* __restrict__ a_,
                                                       float* __restrict__ state, uint16_t* __restrict__ y_) {
    __shared__ float S[64][65];
    __shared__ float vec[5][64];                   // w q k z a
    const int bh = blockIdx.x, i = threadIdx.x;
    const size_t vb = (size_t)bh * 64;
    float* sp = state + (size_t)bh * 64 * 64;
    for (int e = i; e < STATE_VECS; e += 64) state_put(S, e, reinterpret_cast<const float4*>(sp)[e]);
    vec[0][i] = fast_exp(-fast_exp(bf16_to_f32(w_[vb + i])));
    vec[1][i] = bf16_to_f32(q_[vb + i]);
    vec[2][i] = bf16_to_f32(k_[vb + i]);
    vec[3][i] = bf16_to_f32(z_[vb + i]);
    vec[4][i] = bf16_to_f32(a_[vb + i]);
    const float vi = bf16_to_f32(v_[vb + i]);
    __syncthreads();
    float sa = 0.f;
#pragma unroll 8
    for (int j = 0; j < 64; ++j) sa = fmaf(S[i][j], vec[3][j], sa);
    float y = 0.f;
#pragma unroll 8
    for (int j = 0; j < 64; ++j) {
        const float s = fmaf(S[i][j], vec[0][j], fmaf(sa, vec[4][j], vec[2][j] * vi));
        S[i][j] = s;
        y = fmaf(s, vec[1][j], y);
    }
    y_[vb + i] = (uint16_t)f32_to_bf16_bits(y);
    __syncthreads();
    for (int e = i; e < STATE_VECS; e += 64) reinterpret_cast<float4*>(sp)[e] = state_get(S, e);
}

}  // namespace

extern "C" int vrwkv_wkv7_step_bf16(int B, int H, const void* w, const void* q, const void* k, const void* v,
                                    const void* z, const void* a, float* state, void* y, void* stream) {
    if (B <= 0 || H <= 0 || hostchk::any_null(w, q, k, v, z, a, state, y)) return VRWKV_EINVAL;       // no cap on B: one workgroup per (b,h)
    if (hostchk::misaligned(state)) return VRWKV_EALIGN;                                               // the vectors are read by element
    hipLaunchKernelGGL(wkv7_step_kernel, dim3((unsigned)(B * H)), dim3(64), 0, (hipStream_t)stream, H,
                       (const uint16_t*)w, (const uint16_t*)q, (const uint16_t*)k, (const uint16_t*)v,
                       (const uint16_t*)z, (const uint16_t*)a, state, (uint16_t*)y);
    return hostchk::finish_launch();
}
