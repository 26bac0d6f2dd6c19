// Fused per-token kernels of the RWKV-6 decode step (stateful generation).  At T = 1 a layer of RWKV_Tmix_x060
// (VisualRWKV-v6/v6.0/src/model.py:92-226; with a carried state v6.xx/src/model.py:137-144) is launch-bound like the RWKV-7 one
// (decode_fused.hip); what is not a GEMV over a weight matrix is done by two kernels:
//
//   ddlerp     : second stage of the five-way data-dependent token shift (RWKV_Tmix_x060.mix): the five rows
//                h + (x_prev - h) (maa_j + hid_j w2_j[:, c]), then x_prev = h.  time_maa_w2 is read as stored, (5, D, C): a channel
//                chunk's reads are contiguous across lanes.  One workgroup per (64 channels, batch row) -- the one owner of those
//                elements of x_prev, which it has read before it writes them.
//   tmix_head  : per (b, head): second stage of the decay LoRA, the WKV6 state step (wkv6_step.hip) on `state` in place with the
//                time_faaaa bonus, GroupNorm ln_x and the multiplication by silu(gate).
//
// Tensors that the module path holds in bf16 are rounded here too (rb()): lo, w_raw, y, the GroupNorm's output and silu(g).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/visualrwkv_hip.h"
#include <gfx950_prims.h>
#include "decode_common.h"
#include "host_checks.h"

namespace {

using namespace decode;

constexpr int D6_MAX_B = 4;
constexpr int D6_MAX_C = 8192;
constexpr int D6_THREADS = 256;
constexpr int D6_SLOTS = D6_THREADS / 8;       // 32 LoRA rows in flight per workgroup: thread (chunk cl, slot ds)
constexpr int D6_PAD = 68;                     // row stride of the partial sums: the slots of a wave start 4 banks apart, rows stay 16-byte aligned

struct DdArgs {
    const uint16_t *h, *hid, *w2;              // (B,C), (B,5 D), (5,D,C)
    uint16_t* x_prev;                          // (B,C): read, then replaced by h
    const uint16_t* maa[5];                    // (C)
    uint16_t* out[5];                          // (B,C)
    int C;
};

// R = D / 32 rows of every w2_j per thread.  Every global load is issued before the first barrier.
template <int R>
__global__ __launch_bounds__(D6_THREADS) void ddlerp_kernel(DdArgs a) {
    __shared__ __attribute__((aligned(16))) float part[5][D6_SLOTS][D6_PAD];      // [j][slot][channel] partial sums over the slot's rows
    __shared__ float part2[5][4][64];          // [j][quarter of the slots][channel]
    constexpr int D = 32 * R;
    const int tid = threadIdx.x, cl = tid & 7, ds = tid >> 3;
    const int b = blockIdx.y, c0 = blockIdx.x * 64, C = a.C;
    vrwkv_u4 w[5][R];
    float hv[5][R];
#pragma unroll
    for (int j = 0; j < 5; ++j)
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const int d = j * D + ds + 32 * i;
            w[j][i] = ld16(a.w2 + (size_t)d * C + c0 + cl * 8);
            hv[j][i] = bf16_to_f32(a.hid[(size_t)b * 5 * D + d]);
        }
    // the epilogue's operands: thread (j = tid / 8 < 5, chunk tid % 8)
    const bool fin = tid < 40;
    const size_t ro = (size_t)b * C + c0 + cl * 8;
    const vrwkv_u4 zero = vrwkv_u4{0, 0, 0, 0};
    const vrwkv_u4 hr = fin ? ld16(a.h + ro) : zero, pr = fin ? ld16(a.x_prev + ro) : zero;
    // selects, not a.maa[ds]: a dynamically indexed kernel-argument array would be copied to scratch memory
    const uint16_t* maa = ds == 0 ? a.maa[0] : ds == 1 ? a.maa[1] : ds == 2 ? a.maa[2] : ds == 3 ? a.maa[3] : a.maa[4];
    uint16_t* outp = ds == 0 ? a.out[0] : ds == 1 ? a.out[1] : ds == 2 ? a.out[2] : ds == 3 ? a.out[3] : a.out[4];
    const vrwkv_u4 mr = fin ? ld16(maa + c0 + cl * 8) : zero;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < R; ++i) {
            float wv[8];
            unpack8(w[j][i], wv);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = fmaf(wv[e], hv[j][i], acc[e]);
        }
        float4* dst = reinterpret_cast<float4*>(&part[j][ds][cl * 8]);
        dst[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
        dst[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
    }
    __syncthreads();
    {
        const int c = tid & 63, q = tid >> 6;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            float s = 0.f;
#pragma unroll
            for (int t = 0; t < D6_SLOTS / 4; ++t) s += part[j][q * (D6_SLOTS / 4) + t][c];
            part2[j][q][c] = s;
        }
    }
    __syncthreads();
    if (fin) {
        const int j = ds;
        float h[8], xp[8], mu[8], o[8];
        unpack8(hr, h); unpack8(pr, xp); unpack8(mr, mu);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = cl * 8 + e;
            const float m = (part2[j][0][c] + part2[j][1][c]) + (part2[j][2][c] + part2[j][3][c]);
            o[e] = fmaf(xp[e] - h[e], mu[e] + m, h[e]);
        }
        *reinterpret_cast<vrwkv_u4*>(outp + ro) = pack8(o);
        if (j == 0) *reinterpret_cast<vrwkv_u4*>(a.x_prev + ro) = hr;
    }
}

struct Head6Args {
    int H, C, Dd;
    const uint16_t *r, *k, *v, *g;             // (B,C); g is the raw gate product
    const uint16_t *hid, *w2;                  // (B,Dd) = tanh(xw time_decay_w1), (Dd,C) = time_decay_w2 as stored
    const uint16_t *td, *u, *ln_w, *ln_b;      // (C): time_decay, time_faaaa, ln_x
    float eps;
    float* state;                              // (B,H,64,64) fp32 [key][value], in place
    uint16_t* out;                             // (B,C)
};

// Thread (c, qd): value column c of the head, key rows [16 qd, 16 qd + 16) of the step; for the LoRA, thread (chunk cl, slot ds) as above.
template <int R>      // Dd / 32
__global__ __launch_bounds__(D6_THREADS) void tmix6_head_kernel(Head6Args p) {
    __shared__ float S[64][65];
    __shared__ __attribute__((aligned(16))) float part[D6_SLOTS][D6_PAD];         // LoRA partial sums
    __shared__ float vec[8][64];               // r k v g td u ln_w ln_b; td becomes the decay
    __shared__ float ypart[4][64];
    const int tid = threadIdx.x, c = tid & 63, qd = uniform_i32(tid >> 6), cl = tid & 7, ds = tid >> 3;
    const int b = blockIdx.x / p.H, h = blockIdx.x % p.H;
    const size_t cb = (size_t)b * p.C + h * 64;          // this head's 64 channels of batch row b
    float* sp = p.state + (size_t)blockIdx.x * 4096;
    float4 st[STATE_VECS / D6_THREADS];
#pragma unroll
    for (int i = 0; i < STATE_VECS / D6_THREADS; ++i) st[i] = reinterpret_cast<const float4*>(sp)[tid + i * D6_THREADS];
    vrwkv_u4 w[R];
    float hv[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const int d = ds + 32 * i;
        w[i] = ld16(p.w2 + (size_t)d * p.C + h * 64 + cl * 8);
        hv[i] = bf16_to_f32(p.hid[(size_t)b * p.Dd + d]);
    }
    if (qd == 1) {                                       // the eight 128-byte vectors: one 16-byte load per lane
        const int m = c >> 3;
        const uint16_t* src = m == 0 ? p.r + cb : m == 1 ? p.k + cb : m == 2 ? p.v + cb : m == 3 ? p.g + cb
                            : m == 4 ? p.td + h * 64 : m == 5 ? p.u + h * 64 : m == 6 ? p.ln_w + h * 64 : p.ln_b + h * 64;
        unpack8(ld16(src + cl * 8), &vec[m][cl * 8]);
    }
    {
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < R; ++i) {
            float wv[8];
            unpack8(w[i], wv);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = fmaf(wv[e], hv[i], acc[e]);
        }
        float4* dst = reinterpret_cast<float4*>(&part[ds][cl * 8]);
        dst[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
        dst[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
    }
#pragma unroll
    for (int i = 0; i < STATE_VECS / D6_THREADS; ++i) state_put(S, tid + i * D6_THREADS, st[i]);
    __syncthreads();
    if (qd == 0) {
        float lo = 0.f;
#pragma unroll 8
        for (int t = 0; t < D6_SLOTS; ++t) lo += part[t][c];
        const float w_raw = rb(rb(lo) + vec[4][c]);      // time_decay + lora: a bf16 tensor on the module path
        vec[4][c] = fast_exp(-fast_exp(w_raw));
    }
    __syncthreads();
    const int i0 = qd * 16;
    const float vj = vec[2][c];
    float y = 0.f;
#pragma unroll
    for (int i = i0; i < i0 + 16; ++i) {
        const float s = S[i][c], kv = vec[1][i] * vj;
        y = fmaf(vec[0][i], fmaf(vec[5][i], kv, s), y);
        S[i][c] = fmaf(s, vec[4][i], kv);
    }
    ypart[qd][c] = y;
    __syncthreads();
    if (qd == 0) {
        y = rb((ypart[0][c] + ypart[1][c]) + (ypart[2][c] + ypart[3][c]));
        float rstd;
        const float dlt = groupnorm64(y, p.eps, rstd);
        const float gn = rb(dlt * rstd * vec[6][c] + vec[7][c]);
        const float g = vec[3][c];
        const float sg = rb(g / (1.f + fast_exp(-g)));
        p.out[cb + c] = (uint16_t)f32_to_bf16_bits(gn * sg);
    }
#pragma unroll
    for (int i = 0; i < STATE_VECS / D6_THREADS; ++i) reinterpret_cast<float4*>(sp)[tid + i * D6_THREADS] = state_get(S, tid + i * D6_THREADS);
}

inline bool bad_width(int C) { return C <= 0 || C % 64 != 0 || C > D6_MAX_C; }

}  // namespace

extern "C" int vrwkv_decode6_ddlerp_bf16(int B, int C, int D, const void* h, void* x_prev, const void* hid, const void* w2,
                                         const void* const* maa, void* const* out, void* stream) {
    if (B <= 0 || B > D6_MAX_B || hostchk::any_null(h, x_prev, hid, w2, maa, out)) return VRWKV_EINVAL;
    if (bad_width(C) || (D != 32 && D != 64)) return VRWKV_ESHAPE;
    DdArgs a{};
    a.h = (const uint16_t*)h; a.x_prev = (uint16_t*)x_prev; a.hid = (const uint16_t*)hid; a.w2 = (const uint16_t*)w2; a.C = C;
    bool off = hostchk::any_misaligned(h, x_prev, hid, w2);
    for (int j = 0; j < 5; ++j) {
        if (hostchk::any_null(maa[j], out[j])) return VRWKV_EINVAL;
        a.maa[j] = (const uint16_t*)maa[j]; a.out[j] = (uint16_t*)out[j];
        off |= hostchk::any_misaligned(maa[j], out[j]);
    }
    if (off) return VRWKV_EALIGN;          // after every NULL of the arrays: EINVAL comes first
    const dim3 grid((unsigned)(C / 64), (unsigned)B), block(D6_THREADS);
    if (D == 32) hipLaunchKernelGGL(ddlerp_kernel<1>, grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(ddlerp_kernel<2>, grid, block, 0, (hipStream_t)stream, a);
    return hostchk::finish_launch();
}

extern "C" int vrwkv_decode6_tmix_head_bf16(int B, int H, int d_decay, const void* r, const void* k, const void* v, const void* g,
                                            const void* hid, const void* w2, const void* time_decay, const void* u, const void* ln_w,
                                            const void* ln_b, float eps, float* state, void* out, void* stream) {
    if (B <= 0 || B > D6_MAX_B || H <= 0 || hostchk::any_null(r, k, v, g, hid, w2, time_decay, u, ln_w, ln_b, state, out)) return VRWKV_EINVAL;
    if (bad_width(H * 64) || (d_decay != 64 && d_decay != 128)) return VRWKV_ESHAPE;
    if (hostchk::any_misaligned(r, k, v, g, hid, w2, time_decay, u, ln_w, ln_b, state, out)) return VRWKV_EALIGN;
    Head6Args p{};
    p.H = H; p.C = H * 64; p.Dd = d_decay;
    p.r = (const uint16_t*)r; p.k = (const uint16_t*)k; p.v = (const uint16_t*)v; p.g = (const uint16_t*)g;
    p.hid = (const uint16_t*)hid; p.w2 = (const uint16_t*)w2; p.td = (const uint16_t*)time_decay; p.u = (const uint16_t*)u;
    p.ln_w = (const uint16_t*)ln_w; p.ln_b = (const uint16_t*)ln_b; p.eps = eps; p.state = state; p.out = (uint16_t*)out;
    const dim3 grid((unsigned)(B * H)), block(D6_THREADS);
    if (d_decay == 64) hipLaunchKernelGGL(tmix6_head_kernel<2>, grid, block, 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(tmix6_head_kernel<4>, grid, block, 0, (hipStream_t)stream, p);
    return hostchk::finish_launch();
}
