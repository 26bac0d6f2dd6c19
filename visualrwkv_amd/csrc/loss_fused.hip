// Cross-entropy over the 65536-token vocabulary + the reference's L2Wrap gradient term, one pass over the logits in
// each direction (VisualRWKV-v7/v7.00/src/model.py:418-434 `training_step`, :257-271 `L2Wrap`).
//
// The reference runs: contiguous copy of the shifted logits, log-softmax forward, NLL, log-softmax backward, a max over
// the vocabulary, a zero-fill of a logits-sized tensor, a scatter and a logits-sized add of the two gradients -- about
// 40 B per logit of HBM traffic (5.5 GB logits at 16 x 2624 tokens) against 2 (forward) + 4 (backward) here.
//   forward : per row  m = max_c x_c (first arg-max kept),  lse = m + log sum_c e^{x_c - m},  loss = lse - x_label
//   backward: dx_c = w_row (e^{x_c - lse} - [c = label]) + [c = argmax] m l2_factor
// w_row already contains the upstream gradient, 1/max(valid_b,1), 1/B and is 0 for ignored rows (label -100 or the
// last position of a sample); the L2Wrap term is NOT scaled by the upstream gradient (the reference returns it as is,
// model.py:270).  One workgroup per row, online soft-max (one read of the row), fp32 arithmetic.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/visualrwkv_hip.h"
#include <gfx950_prims.h>
#include <host_checks.h>

using hostchk::any_null, hostchk::finish_launch;

namespace {

constexpr int CE_THREADS = 256;

struct MS { float m, s; int idx; };
DEVFN MS ms_merge(MS a, MS b) {             // lower index wins ties
    MS r;
    const bool a_ge = a.m > b.m || (a.m == b.m && a.idx <= b.idx);
    r.m = a_ge ? a.m : b.m;
    r.idx = a_ge ? a.idx : b.idx;
    r.s = a.s * fast_exp(a.m - r.m) + b.s * fast_exp(b.m - r.m);
    return r;
}

__global__ __launch_bounds__(CE_THREADS) void ce_fwd_kernel(int V, const uint16_t* __restrict__ logits,
                                                            const long* __restrict__ labels, float* __restrict__ row_loss,
                                                            float* __restrict__ row_max, float* __restrict__ row_lse,
                                                            int* __restrict__ row_arg) {
    __shared__ float sm[CE_THREADS / 64], ss[CE_THREADS / 64];
    __shared__ int si[CE_THREADS / 64];
    const long row = blockIdx.x;
    const uint16_t* x = logits + row * (long)V;
    MS acc{-3.0e38f, 0.f, 0x7fffffff};
    for (int c0 = threadIdx.x * 8; c0 < V; c0 += CE_THREADS * 8) {
        const uint4 u = *reinterpret_cast<const uint4*>(x + c0);
        const float f[8] = {bf16_lo(u.x), bf16_hi(u.x), bf16_lo(u.y), bf16_hi(u.y), bf16_lo(u.z), bf16_hi(u.z), bf16_lo(u.w), bf16_hi(u.w)};
        float m8 = f[0];
        int i8 = 0;
#pragma unroll
        for (int e = 1; e < 8; ++e) if (f[e] > m8) { m8 = f[e]; i8 = e; }
        float s8 = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) s8 += fast_exp(f[e] - m8);
        acc = ms_merge(acc, MS{m8, s8, c0 + i8});
    }
    // wave reduction through LDS-free shuffles (ds_bpermute), then across the 4 waves
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int src = (threadIdx.x & 63) ^ off;
        MS o{lane_bcast(acc.m, src), lane_bcast(acc.s, src), (int)__float_as_uint(lane_bcast(__uint_as_float((uint32_t)acc.idx), src))};
        acc = ms_merge(acc, o);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sm[wave] = acc.m; ss[wave] = acc.s; si[wave] = acc.idx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        MS t{sm[0], ss[0], si[0]};
        for (int w = 1; w < CE_THREADS / 64; ++w) t = ms_merge(t, MS{sm[w], ss[w], si[w]});
        const float lse = t.m + fast_log(t.s);
        const long lab = labels[row];
        row_max[row] = t.m;
        row_lse[row] = lse;
        row_arg[row] = t.idx;
        row_loss[row] = (lab >= 0 && lab < V) ? lse - bf16_to_f32(x[lab]) : 0.f;
    }
}

DEVFN void ce_bwd_row(int V, const uint16_t* __restrict__ x, long lab, float w, float lse, float l2, int arg,
                      uint16_t* __restrict__ d) {
    for (int c0 = threadIdx.x * 8; c0 < V; c0 += CE_THREADS * 8) {
        const uint4 u = *reinterpret_cast<const uint4*>(x + c0);
        const float f[8] = {bf16_lo(u.x), bf16_hi(u.x), bf16_lo(u.y), bf16_hi(u.y), bf16_lo(u.z), bf16_hi(u.z), bf16_lo(u.w), bf16_hi(u.w)};
        float g[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = c0 + e;
            float v = w != 0.f ? w * (fast_exp(f[e] - lse) - (c == lab ? 1.f : 0.f)) : 0.f;
            v += c == arg ? l2 : 0.f;
            g[e] = v;
        }
        *reinterpret_cast<uint4*>(d + c0) = make_uint4(cvt_pk_bf16(g[0], g[1]), cvt_pk_bf16(g[2], g[3]),
                                                       cvt_pk_bf16(g[4], g[5]), cvt_pk_bf16(g[6], g[7]));
    }
}

__global__ __launch_bounds__(CE_THREADS) void ce_bwd_kernel(int V, const uint16_t* __restrict__ logits,
                                                            const long* __restrict__ labels, const float* __restrict__ row_w,
                                                            const float* __restrict__ row_max, const float* __restrict__ row_lse,
                                                            const int* __restrict__ row_arg, float l2_factor,
                                                            uint16_t* __restrict__ dlogits) {
    const long row = blockIdx.x;
    ce_bwd_row(V, logits + row * (long)V, labels[row], row_w[row], row_lse[row], row_max[row] * l2_factor, row_arg[row],
               dlogits + row * (long)V);
}

// ---- the head's backward on labelled rows only (fused.py _HeadCE) ------------------------------------------------------------------
// A row without a label (row_w == 0) has exactly one nonzero logit gradient, c = bf16(max * l2_factor) at its arg-max.  Its share of the
// input gradient is c * W[arg, :] and of the weight gradient c * x_row added to W's row arg; only the labelled rows need the dense
// backward, which runs on a compact (nrows, V) gradient whose row r is source row idx[r].

// compact ce_bwd: row r of dlogits is ce_bwd's row idx[r]; idx[r] < 0 (padding of the compact matrix) is a row of zeros
__global__ __launch_bounds__(CE_THREADS) void ce_bwd_rows_kernel(int V, const uint16_t* __restrict__ logits,
                                                                 const long* __restrict__ labels, const float* __restrict__ row_w,
                                                                 const float* __restrict__ row_max, const float* __restrict__ row_lse,
                                                                 const int* __restrict__ row_arg, float l2_factor,
                                                                 const long* __restrict__ idx, uint16_t* __restrict__ dlogits) {
    const long r = blockIdx.x, src = idx[r];
    uint16_t* d = dlogits + r * (long)V;
    if (src < 0) {
        for (int c0 = threadIdx.x * 8; c0 < V; c0 += CE_THREADS * 8) *reinterpret_cast<uint4*>(d + c0) = make_uint4(0, 0, 0, 0);
        return;
    }
    ce_bwd_row(V, logits + src * (long)V, labels[src], row_w[src], row_lse[src], row_max[src] * l2_factor, row_arg[src], d);
}

DEVFN float l2_coef(float row_max, float l2_factor) { return bf16_lo(cvt_pk_bf16(row_max * l2_factor, 0.f)); }   // ce_bwd's bf16 value

// dx (nrows, C): pos[i] >= 0 -> row pos[i] of the compact input gradient dxc;  -1 -> c_i W[arg_i, :] (one fp32 product, one rounding: what the
// dense GEMM computes for a row whose only nonzero is c_i -- the + 0 turns a -0 product into the +0 the GEMM's sum gives);  < -1 -> zeros.
__global__ __launch_bounds__(CE_THREADS) void head_dx_kernel(int C, const long* __restrict__ pos, const uint16_t* __restrict__ dxc,
                                                             const uint16_t* __restrict__ W, const float* __restrict__ row_max,
                                                             const int* __restrict__ row_arg, float l2_factor, uint16_t* __restrict__ dx) {
    const long i = blockIdx.x, p = pos[i];
    uint16_t* d = dx + i * (long)C;
    if (p >= 0) {
        const uint16_t* s = dxc + p * (long)C;
        for (int c0 = threadIdx.x * 8; c0 < C; c0 += CE_THREADS * 8) *reinterpret_cast<uint4*>(d + c0) = *reinterpret_cast<const uint4*>(s + c0);
    } else if (p == -1) {
        const float c = l2_coef(row_max[i], l2_factor);
        const uint16_t* w = W + (long)row_arg[i] * C;
        for (int c0 = threadIdx.x * 8; c0 < C; c0 += CE_THREADS * 8) {
            const uint4 u = *reinterpret_cast<const uint4*>(w + c0);
            *reinterpret_cast<uint4*>(d + c0) = make_uint4(cvt_pk_bf16(fmaf(c, bf16_lo(u.x), 0.f), fmaf(c, bf16_hi(u.x), 0.f)),
                                                           cvt_pk_bf16(fmaf(c, bf16_lo(u.y), 0.f), fmaf(c, bf16_hi(u.y), 0.f)),
                                                           cvt_pk_bf16(fmaf(c, bf16_lo(u.z), 0.f), fmaf(c, bf16_hi(u.z), 0.f)),
                                                           cvt_pk_bf16(fmaf(c, bf16_lo(u.w), 0.f), fmaf(c, bf16_hi(u.w), 0.f)));
        }
    } else {
        for (int c0 = threadIdx.x * 8; c0 < C; c0 += CE_THREADS * 8) *reinterpret_cast<uint4*>(d + c0) = make_uint4(0, 0, 0, 0);
    }
}

// Sparse L2Wrap weight gradient  dW[v, :] += sum_{p : arg(srow[p]) = v} c_p x[srow[p], :]  over the n rows srow, sorted by arg (stable:
// ascending row inside a group).  Deterministic and without atomics: the sorted list is cut into tiles of L2W_TILE positions; pass 1 sums
// every run of equal arg inside a tile in list order -- a run that starts and ends in the tile is added to dW at once, the fragment of a
// run that came in from the previous tile and ends here goes to P[tile], the fragment still open at the tile's end to Q[tile]; pass 2 adds
// a run that crossed tiles from its fragments in tile order (Q[t0] + ... + Q[t-1] + P[t]).  dW gets fp32(dW) + sum, rounded once more.
constexpr int L2W_TILE = 32;
constexpr int L2W_THREADS = 256;     // 8 columns per thread

DEVFN void load8(const uint16_t* p, float f[8]) {
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    f[0] = bf16_lo(u.x); f[1] = bf16_hi(u.x); f[2] = bf16_lo(u.y); f[3] = bf16_hi(u.y);
    f[4] = bf16_lo(u.z); f[5] = bf16_hi(u.z); f[6] = bf16_lo(u.w); f[7] = bf16_hi(u.w);
}

DEVFN void add_to_row8(uint16_t* d, const float s[8]) {
    float f[8];
    load8(d, f);
    *reinterpret_cast<uint4*>(d) = make_uint4(cvt_pk_bf16(f[0] + s[0], f[1] + s[1]), cvt_pk_bf16(f[2] + s[2], f[3] + s[3]),
                                              cvt_pk_bf16(f[4] + s[4], f[5] + s[5]), cvt_pk_bf16(f[6] + s[6], f[7] + s[7]));
}

__global__ __launch_bounds__(L2W_THREADS) void l2wrap_wgrad_tiles(long n, int C, const long* __restrict__ srow, const uint16_t* __restrict__ x,
                                                                  const float* __restrict__ row_max, const int* __restrict__ row_arg,
                                                                  float l2_factor, uint16_t* __restrict__ dW, float* __restrict__ P,
                                                                  float* __restrict__ Q) {
    __shared__ long s_row[L2W_TILE];
    __shared__ float s_c[L2W_TILE];
    __shared__ int s_arg[L2W_TILE + 1];                          // s_arg[j]: arg of position p0 + j; the entry after the tile's last: -1 at the list end
    const long t = blockIdx.x, p0 = t * L2W_TILE, p1 = p0 + L2W_TILE < n ? p0 + L2W_TILE : n;
    for (int j = threadIdx.x; j <= L2W_TILE; j += L2W_THREADS) {
        const long p = p0 + j;
        if (p < p1) {
            const long r = srow[p];
            s_row[j] = r;
            s_c[j] = l2_coef(row_max[r], l2_factor);
            s_arg[j] = row_arg[r];
        } else if (p == p1) {
            s_arg[j] = p1 < n ? row_arg[srow[p1]] : -1;
        }
    }
    __syncthreads();
    const int col = (blockIdx.y * L2W_THREADS + threadIdx.x) * 8;
    if (col >= C) return;
    bool from_prev = p0 > 0 && row_arg[srow[p0 - 1]] == s_arg[0];
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int len = (int)(p1 - p0);
    for (int j = 0; j < len; ++j) {
        const float c = s_c[j];
        float f[8];
        load8(x + s_row[j] * (long)C + col, f);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = fmaf(c, f[e], acc[e]);
        const int a = s_arg[j];
        if (s_arg[j + 1] == a) continue;                         // the run goes on (at the tile's last position: into Q below)
        if (from_prev) {
            float* o = P + t * (long)C + col;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = acc[e];
        } else {
            add_to_row8(dW + (long)a * C + col, acc);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.f;
        from_prev = false;
    }
    if (s_arg[len] == s_arg[len - 1]) {                          // the last run goes on in the next tile
        float* o = Q + t * (long)C + col;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = acc[e];
    }
}

__global__ __launch_bounds__(L2W_THREADS) void l2wrap_wgrad_join(long n, int C, const long* __restrict__ srow, const int* __restrict__ row_arg,
                                                                 uint16_t* __restrict__ dW, const float* __restrict__ P,
                                                                 const float* __restrict__ Q) {
    const long t = blockIdx.x, p0 = t * L2W_TILE, p1 = p0 + L2W_TILE < n ? p0 + L2W_TILE : n;
    const int col = (blockIdx.y * L2W_THREADS + threadIdx.x) * 8;
    if (t == 0 || col >= C) return;
    const int v = row_arg[srow[p0]];
    if (row_arg[srow[p0 - 1]] != v) return;                     // no run comes in from the previous tile
    if (p1 < n && row_arg[srow[p1]] == v) return;               // ... or it goes on past this one: a later tile adds it
    long t0 = t - 1;
    while (t0 > 0 && row_arg[srow[t0 * L2W_TILE - 1]] == v) --t0;
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (long k = t0; k <= t; ++k) {
        const float* q = (k < t ? Q : P) + k * (long)C + col;
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] += q[e];
    }
    add_to_row8(dW + (long)v * C + col, s);
}

}  // namespace

extern "C" {

int vrwkv_ce_fwd_bf16(long nrows, int V, const void* logits, const long* labels, float* row_loss, float* row_max,
                      float* row_lse, int* row_argmax, void* stream) {
    if (nrows <= 0 || any_null(logits, labels, row_loss, row_max, row_lse, row_argmax)) return VRWKV_EINVAL;
    if (V <= 0 || V % 8 != 0) return VRWKV_ESHAPE;
    hipLaunchKernelGGL(ce_fwd_kernel, dim3((unsigned)nrows), dim3(CE_THREADS), 0, (hipStream_t)stream, V,
                       (const uint16_t*)logits, labels, row_loss, row_max, row_lse, row_argmax);
    return finish_launch();
}

int vrwkv_ce_bwd_bf16(long nrows, int V, const void* logits, const long* labels, const float* row_w, const float* row_max,
                      const float* row_lse, const int* row_argmax, float l2_factor, void* dlogits, void* stream) {
    if (nrows <= 0 || any_null(logits, labels, row_w, row_max, row_lse, row_argmax, dlogits)) return VRWKV_EINVAL;
    if (V <= 0 || V % 8 != 0) return VRWKV_ESHAPE;
    hipLaunchKernelGGL(ce_bwd_kernel, dim3((unsigned)nrows), dim3(CE_THREADS), 0, (hipStream_t)stream, V,
                       (const uint16_t*)logits, labels, row_w, row_max, row_lse, row_argmax, l2_factor, (uint16_t*)dlogits);
    return finish_launch();
}

int vrwkv_ce_bwd_rows_bf16(long nrows, int V, const void* logits, const long* labels, const float* row_w, const float* row_max,
                           const float* row_lse, const int* row_argmax, float l2_factor, const long* idx, void* dlogits, void* stream) {
    if (nrows <= 0 || any_null(logits, labels, row_w, row_max, row_lse, row_argmax, idx, dlogits)) return VRWKV_EINVAL;
    if (V <= 0 || V % 8 != 0) return VRWKV_ESHAPE;
    hipLaunchKernelGGL(ce_bwd_rows_kernel, dim3((unsigned)nrows), dim3(CE_THREADS), 0, (hipStream_t)stream, V, (const uint16_t*)logits,
                       labels, row_w, row_max, row_lse, row_argmax, l2_factor, idx, (uint16_t*)dlogits);
    return finish_launch();
}

int vrwkv_head_dx_bf16(long nrows, int C, const long* pos, const void* dxc, const void* W, const float* row_max, const int* row_argmax,
                       float l2_factor, void* dx, void* stream) {
    if (nrows <= 0 || any_null(pos, W, row_max, row_argmax, dx)) return VRWKV_EINVAL;     // dxc: NULL when no row has pos >= 0
    if (C <= 0 || C % 8 != 0) return VRWKV_ESHAPE;
    hipLaunchKernelGGL(head_dx_kernel, dim3((unsigned)nrows), dim3(CE_THREADS), 0, (hipStream_t)stream, C, pos, (const uint16_t*)dxc,
                       (const uint16_t*)W, row_max, row_argmax, l2_factor, (uint16_t*)dx);
    return finish_launch();
}

long vrwkv_l2wrap_wgrad_ws_floats(long n, int C) {
    if (n < 0 || C <= 0 || C % 8 != 0) return -1;
    return 2 * ((n + L2W_TILE - 1) / L2W_TILE) * (long)C;
}

int vrwkv_l2wrap_wgrad_bf16(long n, int C, const long* srow, const void* x, const float* row_max, const int* row_argmax, float l2_factor,
                            void* dW, float* ws, void* stream) {
    if (n < 0 || any_null(srow, x, row_max, row_argmax, dW, ws)) return VRWKV_EINVAL;
    if (C <= 0 || C % 8 != 0) return VRWKV_ESHAPE;
    if (n == 0) return VRWKV_OK;
    const long tiles = (n + L2W_TILE - 1) / L2W_TILE;
    float* P = ws;
    float* Q = ws + tiles * (long)C;
    const dim3 grid((unsigned)tiles, (unsigned)((C / 8 + L2W_THREADS - 1) / L2W_THREADS));
    hipLaunchKernelGGL(l2wrap_wgrad_tiles, grid, dim3(L2W_THREADS), 0, (hipStream_t)stream, n, C, srow, (const uint16_t*)x, row_max,
                       row_argmax, l2_factor, (uint16_t*)dW, P, Q);
    if (int rc = finish_launch()) return rc;
    hipLaunchKernelGGL(l2wrap_wgrad_join, grid, dim3(L2W_THREADS), 0, (hipStream_t)stream, n, C, srow, row_argmax, (uint16_t*)dW,
                       (const float*)P, (const float*)Q);
    return finish_launch();
}

}  // extern "C"
