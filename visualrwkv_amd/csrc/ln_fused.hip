// Residual add + LayerNorm, forward and backward, one pass each (RWKV-7 Block: x = x + att(ln1(x)); x = x + ffn(ln2(x)),
// VisualRWKV-v7/v7.00/src/model.py:247-254, and ln_out, :318).
//
//   forward :  xn = bf16(x + delta)            (skipped when delta == nullptr: xn = x)
//              y  = (xn - mean) * rstd * w + b  with the statistics of the ROUNDED xn (what the reference's separate
//                                               bf16 add followed by nn.LayerNorm sees), fp32 arithmetic, one rounding
//   backward:  dx = dres + rstd * (g - mean(g) - xhat * mean(g * xhat)),  g = dy * w,  xhat = (xn - mean) * rstd
//              dw = sum_rows dy * xhat,  db = sum_rows dy
// The reference runs these as separate eager kernels (add, LayerNorm forward, LayerNorm backward x3, gradient add):
// 13 B/element forward and ~24 B/element backward against 8 + 8 here.
//
// A workgroup owns a contiguous range of token rows and walks it row by row; a thread owns 8 consecutive channels
// (16-byte accesses), so the per-channel parameter gradients stay in registers for the whole range and leave as one
// fp32 partial row per workgroup (summed by colsum_kernel in a fixed order: deterministic, no atomics).  Row
// statistics: DPP wave all-reduce, then one LDS slot per wave (double buffered by row parity -> one barrier per
// reduction).  The next row's loads are issued before the current row is reduced.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/visualrwkv_hip.h"
#include <gfx950_prims.h>
#include <host_checks.h>
#include <ln_kernels.h>

namespace {

using namespace vln;

#ifndef VRWKV_LN_BWD_GRID
#define VRWKV_LN_BWD_GRID 1024
#endif
#ifndef VRWKV_LN_MIX_BWD_GRID
#define VRWKV_LN_MIX_BWD_GRID 768
#endif
// Forward kernels: MANY short-lived workgroups keep more requests in flight than 2048 resident ones that walk 20 rows each
// (profiles/r4_eltwise_micro_ab.jsonl): add + LayerNorm one row per workgroup (-20 %), the lerp kernels four (the shifted row
// x[n-1] is the previous iteration's row in registers: with one row per workgroup it would be read and normalised twice)
constexpr int LN_ROWS_PER_WG = 1, LN_MIX_ROWS_PER_WG = 4;
inline int ln_grid(long ntok, int rows = LN_ROWS_PER_WG) {
    const long g = (ntok + rows - 1) / rows;
    return (int)(g < 1 ? 1 : g > (1L << 22) ? (1L << 22) : g);
}
// Backward kernels: one workgroup per resident slot (add_ln_bwd: 104 VGPRs, 4 workgroups of 256 threads per CU; ln_mix_bwd<1>: 162, 3 per
// CU) -- a single round of equal token ranges, and half / a third of the partial rows for ln_colsum_kernel to read (2048 rows cost
// 46 us per call, 2.3 ms per step)
constexpr int LN_BWD_GRID = VRWKV_LN_BWD_GRID, LN_MIX_BWD_GRID = VRWKV_LN_MIX_BWD_GRID;
inline int ln_bwd_grid(long ntok) { return (int)(ntok < LN_BWD_GRID ? ntok : LN_BWD_GRID); }
inline int ln_mix_bwd_grid(long ntok) { return (int)(ntok < LN_MIX_BWD_GRID ? ntok : LN_MIX_BWD_GRID); }
// The compressor's tail: one workgroup per pooled output (a window of Lin / Lout rows, walked with the next row in flight) up to the cap, then
// contiguous ranges of outputs
constexpr int LN_POOL_FWD_GRID = 1024;
inline int ln_pool_grid(long nout) { return (int)(nout < LN_POOL_FWD_GRID ? nout : LN_POOL_FWD_GRID); }
inline int ln_ok(int C) { return C > 0 && C % 64 == 0 && C <= 8192; }
inline int ln_threads(int C) { return (C / 8 + 63) / 64 * 64; }
inline void colsum(int G, long width, const float* part, float* out, hipStream_t st) {
    hipLaunchKernelGGL(ln_colsum_kernel, dim3((unsigned)(width / 16)), dim3(256), 0, st, G, width, part, out);
}
using hostchk::finish_launch;

// The ln_mix kernels' host side: one description of a launch each way, the variants (the kernels' PK / CARRY / ROUTED flags) its optional
// fields -- left NULL they select the plain kernel (route: the kernels' own LmRoute).  The vrwkv_ln_mix_* entries below fill one and call
// ln_mix_fwd / ln_mix_bwd, which validate, pick the instantiation and, in the backward, sum the per-workgroup partial rows.
inline bool route_ok(const LmRoute& r) { return r.w1 && r.b1 && r.mu1 && r.sel && r.pos; }
struct LnMixFwd {
    long ntok; int T, C; float eps; int M;
    const void *x, *delta, *w, *b; const void* const* mu;
    void* xn; void* const* out; float *mean, *rstd;
    void* stream;
    const unsigned char* first = nullptr;                       // PK
    const void* y_prev = nullptr; void* y_last = nullptr;       // CARRY
    const LmRoute* route = nullptr;                             // ROUTED (M = 1; mu[0], out[0]: expert 0's lerp, the routed tensor)
    bool carry() const { return y_prev || y_last; }
};
struct LnMixBwd {                                               // M = 1 only, see vrwkv_ln_mix_bwd_bf16
    long ntok; int T, C, M;
    const void* xn; const float *mean, *rstd; const void *w, *b; const void* const* mu;
    const void* const* dout; const void* dout3_second; const void* dres;
    void* dx; float *dwb, *dmu, *ws;
    void* stream;
    const unsigned char* first = nullptr;                                                       // PK
    const void* y_prev = nullptr; const float* dy_last = nullptr; float* dy_prev = nullptr;     // CARRY
    const LmRoute* route = nullptr;                                                             // ROUTED (dout[0]: in routed row order)
    bool carry() const { return y_prev || dy_last || dy_prev; }
};
struct LnMixParts { int G; float *ln, *mu; };                   // the backward's grid and its two runs of partial rows in ws

// One variant's kernel: the forward by M (routed rows: M = 1 only), the backward by its launch bound (routed rows stop at C = 4096: no 1024)
template <bool PK, bool CARRY, bool ROUTED>
void ln_mix_fwd_launch(const LnMixFwd& a, const LmPtrs& pm, const LmOuts& po) {
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(ln_grid(a.ntok, LN_MIX_ROWS_PER_WG)), dim3(ln_threads(a.C)), 0, (hipStream_t)a.stream, a.ntok, a.T, a.C, a.eps,
                           (const uint16_t*)a.x, (const uint16_t*)a.delta, (const uint16_t*)a.w, (const uint16_t*)a.b, (uint16_t*)a.xn, a.mean, a.rstd, pm, po,
                           a.first, (const uint16_t*)a.y_prev, (uint16_t*)a.y_last, a.route ? *a.route : LmRoute());
    };
    if (ROUTED || a.M == 1) go(ln_mix_fwd_kernel<1, PK, CARRY, ROUTED>);
    else if constexpr (!ROUTED) go(ln_mix_fwd_kernel<6, PK, CARRY, ROUTED>);
}
template <bool PK, bool CARRY, bool ROUTED>
void ln_mix_bwd_launch(const LnMixBwd& a, const LmPtrs& pm, const LmPtrs& pd, const LnMixParts& part) {
    const int threads = ln_threads(a.C);
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(part.G), dim3(threads), 0, (hipStream_t)a.stream, a.ntok, a.T, a.C, (const uint16_t*)a.xn, a.mean, a.rstd,
                           (const uint16_t*)a.w, (const uint16_t*)a.b, pm, pd, (const uint16_t*)a.dout3_second, (const uint16_t*)a.dres, (uint16_t*)a.dx,
                           part.ln, part.mu, a.first, (const uint16_t*)a.y_prev, a.dy_last, a.dy_prev, a.route ? *a.route : LmRoute());
    };
    if (threads <= 256) go(ln_mix_bwd_kernel<1, false, 256, PK, CARRY, ROUTED>);
    else if (ROUTED || threads <= 512) go(ln_mix_bwd_kernel<1, false, 512, PK, CARRY, ROUTED>);
    else if constexpr (!ROUTED) go(ln_mix_bwd_kernel<1, false, 1024, PK, CARRY, ROUTED>);
}
// The variant from the fields.  PK with CARRY, and ROUTED with CARRY, are not built: the launchers refuse them before they come here.  Four
// functions in this order, not two: kernels enter the code object in the order of their first mention, and this is the order they have there.
void ln_mix_fwd_rows(const LnMixFwd& a, const LmPtrs& pm, const LmOuts& po) {
    if (a.first) ln_mix_fwd_launch<true, false, false>(a, pm, po);
    else if (!a.carry()) ln_mix_fwd_launch<false, false, false>(a, pm, po);
    else ln_mix_fwd_launch<false, true, false>(a, pm, po);
}
void ln_mix_bwd_rows(const LnMixBwd& a, const LmPtrs& pm, const LmPtrs& pd, const LnMixParts& part) {
    if (a.first) ln_mix_bwd_launch<true, false, false>(a, pm, pd, part);
    else if (!a.carry()) ln_mix_bwd_launch<false, false, false>(a, pm, pd, part);
    else ln_mix_bwd_launch<false, true, false>(a, pm, pd, part);
}
void ln_mix_fwd_routed(const LnMixFwd& a, const LmPtrs& pm, const LmOuts& po) {
    if (a.first) ln_mix_fwd_launch<true, false, true>(a, pm, po); else ln_mix_fwd_launch<false, false, true>(a, pm, po);
}
void ln_mix_bwd_routed(const LnMixBwd& a, const LmPtrs& pm, const LmPtrs& pd, const LnMixParts& part) {
    if (a.first) ln_mix_bwd_launch<true, false, true>(a, pm, pd, part); else ln_mix_bwd_launch<false, false, true>(a, pm, pd, part);
}

int ln_mix_fwd(const LnMixFwd& a) {
    if (a.ntok <= 0 || a.T <= 0 || a.ntok % a.T != 0 || !a.x || !a.w || !a.b || !a.mu || !a.out || !a.mean || !a.rstd || (a.delta && !a.xn)) return VRWKV_EINVAL;
    if (a.route && (!route_ok(*a.route) || !a.mu[0] || !a.out[0])) return VRWKV_EINVAL;
    if (a.carry() && (a.first || a.route)) return VRWKV_EINVAL;         // not built
    if (!ln_ok(a.C) || (a.M != 1 && a.M != 6) || (a.route && (a.M != 1 || a.C > 4096))) return VRWKV_ESHAPE;
    LmPtrs pm{}; LmOuts po{};
    for (int j = 0; j < a.M; ++j) {
        if (!a.mu[j] || !a.out[j]) return VRWKV_EINVAL;
        pm.p[j] = (const uint16_t*)a.mu[j]; po.p[j] = (uint16_t*)a.out[j];
    }
    if (a.route) ln_mix_fwd_routed(a, pm, po); else ln_mix_fwd_rows(a, pm, po);
    return finish_launch();
}

// ws: G (2 + M) C floats, routed G (4 + 2) C -- the (dgamma, dbeta) partial rows of every workgroup, then its dmu rows
int ln_mix_bwd(const LnMixBwd& a) {
    if (a.ntok <= 0 || a.T <= 0 || a.ntok % a.T != 0 || !a.xn || !a.mean || !a.rstd || !a.w || !a.b || !a.mu || !a.dout || !a.dx || !a.dwb || !a.dmu || !a.ws)
        return VRWKV_EINVAL;
    if (a.route && (!route_ok(*a.route) || !a.mu[0] || !a.dout[0])) return VRWKV_EINVAL;
    if (a.carry() && (a.first || a.route)) return VRWKV_EINVAL;         // not built
    // M = 6: vrwkv_mix_bwd_ln_bf16 / _packed / _carry (tmix_fused.hip) + vrwkv_add_ln_bwd_bf16
    if (!ln_ok(a.C) || a.M != 1 || a.dout3_second || (a.route && a.C > 4096)) return VRWKV_ESHAPE;
    if (!a.mu[0] || !a.dout[0]) return VRWKV_EINVAL;
    LmPtrs pm{}, pd{};
    pm.p[0] = (const uint16_t*)a.mu[0]; pd.p[0] = (const uint16_t*)a.dout[0];
    const int G = ln_mix_bwd_grid(a.ntok);
    const long w_ln = (a.route ? 4L : 2L) * a.C, w_mu = (a.route ? 2L : 1L) * a.C;
    const LnMixParts part{G, a.ws, a.ws + (size_t)G * w_ln};
    if (a.route) ln_mix_bwd_routed(a, pm, pd, part); else ln_mix_bwd_rows(a, pm, pd, part);
    colsum(G, w_ln, part.ln, a.dwb, (hipStream_t)a.stream);
    colsum(G, w_mu, part.mu, a.dmu, (hipStream_t)a.stream);
    return finish_launch();
}

}  // namespace

extern "C" {

long vrwkv_add_ln_ws_floats(long ntok, int C) { return (long)ln_bwd_grid(ntok) * 2 * C; }

int vrwkv_add_ln_fwd_bf16(long ntok, int C, float eps, const void* x, const void* delta, const void* w, const void* b,
                          void* xn, void* y, float* mean, float* rstd, void* stream) {
    if (ntok <= 0 || !x || !w || !b || !y || !mean || !rstd || (delta && !xn)) return VRWKV_EINVAL;
    if (!ln_ok(C)) return VRWKV_ESHAPE;
    hipLaunchKernelGGL(add_ln_fwd_kernel, dim3(ln_grid(ntok)), dim3(ln_threads(C)), 0, (hipStream_t)stream, ntok, C, eps,
                       (const uint16_t*)x, (const uint16_t*)delta, (const uint16_t*)w, (const uint16_t*)b, (uint16_t*)xn,
                       (uint16_t*)y, mean, rstd, (const long*)nullptr, (const uint16_t*)nullptr);
    return finish_launch();
}

// Inference form for the frozen ViT towers (timm pre-LN blocks, src/vision.py:123-134; SAM blocks, src/sam.py:231-247):
// xn = x + delta * dscale (dscale: LayerScale gamma, may be NULL), y = LayerNorm(xn); no statistics are kept.
int vrwkv_add_ln_scaled_fwd_bf16(long ntok, int C, float eps, const void* x, const void* delta, const void* dscale, const void* w,
                                 const void* b, void* xn, void* y, void* stream) {
    if (ntok <= 0 || !x || !w || !b || !y || (delta && !xn) || (dscale && !delta)) return VRWKV_EINVAL;
    if (!ln_ok(C)) return VRWKV_ESHAPE;
    hipLaunchKernelGGL(add_ln_fwd_kernel, dim3(ln_grid(ntok)), dim3(ln_threads(C)), 0, (hipStream_t)stream, ntok, C, eps,
                       (const uint16_t*)x, (const uint16_t*)delta, (const uint16_t*)w, (const uint16_t*)b, (uint16_t*)xn,
                       (uint16_t*)y, (float*)nullptr, (float*)nullptr, (const long*)nullptr, (const uint16_t*)dscale);
    return finish_launch();
}

// LayerNorm of the projector output written straight into the rows of the token-embedding tensor that hold the image
// placeholders (MLPWithContextGating's ln_v + the masked scatter of preparing_embedding, src/model.py:338,485-493):
// out[row_index[n]] = LN(x[n]).  row_index: device int64, distinct rows; a NEGATIVE entry drops feature row n (the sample
// had fewer placeholders than features -- the reference truncates the features, src/model.py:487-491): nothing is written
// for it and in the backward it receives a zero gradient and does not contribute to dgamma / dbeta.
int vrwkv_ln_scatter_fwd_bf16(long ntok, int C, float eps, const void* x, const void* w, const void* b, const long* row_index,
                              void* out, float* mean, float* rstd, void* stream) {
    if (ntok <= 0 || !x || !w || !b || !row_index || !out || !mean || !rstd) return VRWKV_EINVAL;
    if (!ln_ok(C)) return VRWKV_ESHAPE;
    hipLaunchKernelGGL(add_ln_fwd_kernel, dim3(ln_grid(ntok)), dim3(ln_threads(C)), 0, (hipStream_t)stream, ntok, C, eps,
                       (const uint16_t*)x, (const uint16_t*)nullptr, (const uint16_t*)w, (const uint16_t*)b, (uint16_t*)nullptr,
                       (uint16_t*)out, mean, rstd, row_index, (const uint16_t*)nullptr);
    return finish_launch();
}

// ... and its backward: dx[n] = LN'(dout[row_index[n]]), dwb = (dgamma, dbeta); ws as for vrwkv_add_ln_bwd_bf16
int vrwkv_ln_gather_bwd_bf16(long ntok, int C, const void* dout, const long* row_index, const void* x, const float* mean,
                             const float* rstd, const void* w, void* dx, float* dwb, float* ws, void* stream) {
    if (ntok <= 0 || !dout || !row_index || !x || !mean || !rstd || !w || !dx || !dwb || !ws) return VRWKV_EINVAL;
    if (!ln_ok(C)) return VRWKV_ESHAPE;
    const int G = ln_bwd_grid(ntok);
    hipLaunchKernelGGL(add_ln_bwd_kernel, dim3(G), dim3(ln_threads(C)), 0, (hipStream_t)stream, ntok, C, (const uint16_t*)dout,
                       (const uint16_t*)nullptr, (const uint16_t*)x, mean, rstd, (const uint16_t*)w, (uint16_t*)dx, ws, row_index);
    colsum(G, 2L * C, ws, dwb, (hipStream_t)stream);
    return finish_launch();
}

// The visual token compressor's tail: ln_out, unpad, AdaptiveAvgPool1d over tokens and the scatter into the placeholder rows in one pass
// (VisualRWKV-v7/v7.04/src/model.py:372-373,524-529,544-552); see ln_pool_fwd_kernel.  The backward's ws: vrwkv_add_ln_ws_floats(B T, C).
int vrwkv_ln_pool_scatter_fwd_bf16(int B, int T, int pad, int Lout, int C, float eps, const void* x, const void* delta, const void* w,
                                   const void* b, const long* row_index, void* xn, void* out, float* mean, float* rstd, void* stream) {
    if (B <= 0 || T <= 0 || pad < 0 || pad >= T || !x || !w || !b || !out || !mean || !rstd || (delta && !xn)) return VRWKV_EINVAL;
    if (!ln_ok(C) || Lout < 1 || Lout > T - pad) return VRWKV_ESHAPE;
    hipLaunchKernelGGL(ln_pool_fwd_kernel, dim3(ln_pool_grid((long)B * Lout)), dim3(ln_threads(C)), 0, (hipStream_t)stream, B, T, pad, Lout, C, eps,
                       (const uint16_t*)x, (const uint16_t*)delta, (const uint16_t*)w, (const uint16_t*)b, (uint16_t*)xn, (uint16_t*)out, mean, rstd,
                       row_index);
    return finish_launch();
}

int vrwkv_ln_pool_gather_bwd_bf16(int B, int T, int pad, int Lout, int C, const void* dout, const long* row_index, const void* xn,
                                  const float* mean, const float* rstd, const void* w, void* dx, float* dwb, float* ws, void* stream) {
    if (B <= 0 || T <= 0 || pad < 0 || pad >= T || !dout || !xn || !mean || !rstd || !w || !dx || !dwb || !ws) return VRWKV_EINVAL;
    if (!ln_ok(C) || Lout < 1 || Lout > T - pad) return VRWKV_ESHAPE;
    const int G = ln_bwd_grid((long)B * T);
    hipLaunchKernelGGL(ln_pool_bwd_kernel, dim3(G), dim3(ln_threads(C)), 0, (hipStream_t)stream, B, T, pad, Lout, C, (const uint16_t*)dout, row_index,
                       (const uint16_t*)xn, mean, rstd, (const uint16_t*)w, (uint16_t*)dx, ws);
    colsum(G, 2L * C, ws, dwb, (hipStream_t)stream);
    return finish_launch();
}

// The RWKV vision encoder's tail: ln_out over all rows scattered into the placeholder rows, and the ImageNet head's mean over tokens of the same
// rows, one read of the residual stream each way (VisualRWKV-v7/v7.10/src/model.py:392-394,510-526); see ln_scatter_mean_fwd_kernel.
// ws (both ways): vrwkv_ln_scatter_mean_ws_floats(B, L, C) floats -- the forward's per-range partial sums / the backward's (dgamma, dbeta) rows.
constexpr int LN_MEAN_ROWS = 8, LN_MEAN_PARTS = 64;         // rows a forward workgroup walks, and the cap on partial rows per sample
inline int ln_mean_parts(int L) { const int p = (L + LN_MEAN_ROWS - 1) / LN_MEAN_ROWS; return p < LN_MEAN_PARTS ? p : LN_MEAN_PARTS; }

long vrwkv_ln_scatter_mean_ws_floats(int B, int L, int C) {
    if (B <= 0 || L <= 0 || !ln_ok(C) || (long)B * ln_mean_parts(L) >= (1L << 31)) return -1;
    const long f = (long)B * ln_mean_parts(L) * C, bw = vrwkv_add_ln_ws_floats((long)B * L, C);
    return f > bw ? f : bw;
}

int vrwkv_ln_scatter_mean_fwd_bf16(int B, int L, int C, float eps, const void* x, const void* delta, const void* w, const void* b,
                                   const long* row_index, void* xn, void* out, void* pooled, float* mean, float* rstd, float* ws, void* stream) {
    if (B <= 0 || L <= 0 || !x || !w || !b || !out || !pooled || !mean || !rstd || !ws || (delta && !xn)) return VRWKV_EINVAL;
    if (!ln_ok(C) || (long)B * ln_mean_parts(L) >= (1L << 31)) return VRWKV_ESHAPE;
    const int P = ln_mean_parts(L);
    hipLaunchKernelGGL(ln_scatter_mean_fwd_kernel, dim3((unsigned)(B * P)), dim3(ln_threads(C)), 0, (hipStream_t)stream, L, P, C, eps, (const uint16_t*)x,
                       (const uint16_t*)delta, (const uint16_t*)w, (const uint16_t*)b, (uint16_t*)xn, (uint16_t*)out, mean, rstd, row_index, ws);
    const long n = (long)B * C;
    hipLaunchKernelGGL(ln_mean_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, P, C, 1.f / (float)L, ws,
                       (const uint16_t*)w, (const uint16_t*)b, (uint16_t*)pooled);
    return finish_launch();
}

// dout (rows of the scattered tensor) and dpooled (B, C) bf16: either may be NULL, not both; row_index NULL: dout is (B L, C) in order.
// dx (B, L, C) bf16, dwb (2 C fp32) = (dgamma, dbeta), written.  With dpooled == NULL this is vrwkv_ln_gather_bwd_bf16 bit for bit.
int vrwkv_ln_gather_mean_bwd_bf16(int B, int L, int C, const void* dout, const long* row_index, const void* dpooled, const void* xn,
                                  const float* mean, const float* rstd, const void* w, void* dx, float* dwb, float* ws, void* stream) {
    if (B <= 0 || L <= 0 || (!dout && !dpooled) || !xn || !mean || !rstd || !w || !dx || !dwb || !ws) return VRWKV_EINVAL;
    if (!ln_ok(C)) return VRWKV_ESHAPE;
    const long ntok = (long)B * L;
    const int G = ln_bwd_grid(ntok);
    hipLaunchKernelGGL(ln_gather_mean_bwd_kernel, dim3(G), dim3(ln_threads(C)), 0, (hipStream_t)stream, ntok, L, C, (const uint16_t*)dout, row_index,
                       (const uint16_t*)dpooled, (const uint16_t*)xn, mean, rstd, (const uint16_t*)w, (uint16_t*)dx, ws);
    colsum(G, 2L * C, ws, dwb, (hipStream_t)stream);
    return finish_launch();
}

int vrwkv_add_ln_bwd_bf16(long ntok, int C, const void* dy, const void* dres, const void* xn, const float* mean,
                          const float* rstd, const void* w, void* dx, float* dwb, float* ws, void* stream) {
    if (ntok <= 0 || !dy || !xn || !mean || !rstd || !w || !dx || !dwb || !ws) return VRWKV_EINVAL;
    if (!ln_ok(C)) return VRWKV_ESHAPE;
    const int G = ln_bwd_grid(ntok);
    hipLaunchKernelGGL(add_ln_bwd_kernel, dim3(G), dim3(ln_threads(C)), 0, (hipStream_t)stream, ntok, C, (const uint16_t*)dy,
                       (const uint16_t*)dres, (const uint16_t*)xn, mean, rstd, (const uint16_t*)w, (uint16_t*)dx, ws, (const long*)nullptr);
    colsum(G, 2L * C, ws, dwb, (hipStream_t)stream);
    return finish_launch();
}

// Residual add + LayerNorm + token shift + M lerps (M = 1: channel-mix, M = 6: time-mix), see ln_mix_fwd_kernel above.
long vrwkv_ln_mix_ws_floats(long ntok, int C, int M) { return (long)ln_mix_bwd_grid(ntok) * (2 + M) * C; }

int vrwkv_ln_mix_fwd_bf16(long ntok, int T, int C, float eps, int M, const void* x, const void* delta, const void* w, const void* b,
                          const void* const* mu, void* xn, void* const* out, float* mean, float* rstd, void* stream) {
    return ln_mix_fwd({ntok, T, C, eps, M, x, delta, w, b, mu, xn, out, mean, rstd, stream});
}

// the same with sample boundaries inside the rows: first[n] != 0 (ntok bytes) = row n reads zeros for its shifted value; NULL = the entry above
int vrwkv_ln_mix_fwd_packed_bf16(long ntok, int T, int C, float eps, int M, const void* x, const void* delta, const void* w, const void* b,
                                 const void* const* mu, void* xn, void* const* out, float* mean, float* rstd, const unsigned char* first,
                                 void* stream) {
    return ln_mix_fwd({ntok, T, C, eps, M, x, delta, w, b, mu, xn, out, mean, rstd, stream, first});
}

// the same for one segment of a longer row (training across a cut): y_prev (B, C) bf16 = the LayerNorm output of the row before each sample's
// first row (NULL = zeros), y_last (B, C) bf16 receives the LayerNorm output of each sample's last row (NULL = not wanted).  Both NULL = the
// plain entry.
int vrwkv_ln_mix_fwd_carry_bf16(long ntok, int T, int C, float eps, int M, const void* x, const void* delta, const void* w, const void* b,
                                const void* const* mu, void* xn, void* const* out, float* mean, float* rstd, const void* y_prev, void* y_last,
                                void* stream) {
    return ln_mix_fwd({ntok, T, C, eps, M, x, delta, w, b, mu, xn, out, mean, rstd, stream, nullptr, y_prev, y_last});
}

// dx = dres + LN'(gradient of the lerps' input), dwb = (dgamma, dbeta) (2, C) fp32, dmu (M, C) fp32; dres may be NULL;
// ws: vrwkv_ln_mix_ws_floats(ntok, C, M) floats.  M = 1 only: with six lerps the kernel keeps ~200 values per thread (48 gradient
// accumulators, the prefetched rows) and hipcc spills inside the token loop at two workgroups per CU (1.02 ms against 0.72 ms for
// the two kernels); the time-mix backward is vrwkv_mix_bwd_ln_bf16 (tmix_fused.hip) followed by vrwkv_add_ln_bwd_bf16.
int vrwkv_ln_mix_bwd_bf16(long ntok, int T, int C, int M, const void* xn, const float* mean, const float* rstd, const void* w,
                          const void* b, const void* const* mu, const void* const* dout, const void* dout3_second, const void* dres,
                          void* dx, float* dwb, float* dmu, float* ws, void* stream) {
    return ln_mix_bwd({ntok, T, C, M, xn, mean, rstd, w, b, mu, dout, dout3_second, dres, dx, dwb, dmu, ws, stream});
}

// the same with sample boundaries inside the rows: first[n] != 0 (ntok bytes) = no gradient from row n to row n-1; NULL = the entry above
int vrwkv_ln_mix_bwd_packed_bf16(long ntok, int T, int C, int M, const void* xn, const float* mean, const float* rstd, const void* w,
                                 const void* b, const void* const* mu, const void* const* dout, const void* dout3_second, const void* dres,
                                 const unsigned char* first, void* dx, float* dwb, float* dmu, float* ws, void* stream) {
    return ln_mix_bwd({ntok, T, C, M, xn, mean, rstd, w, b, mu, dout, dout3_second, dres, dx, dwb, dmu, ws, stream, first});
}

// the channel-mix backward for one segment of a longer row: y_prev as in the forward; dy_last (B, C) fp32 = the gradient the next segment sends
// to the LayerNorm output of each sample's last row (NULL = none), dy_prev (B, C) fp32 receives the gradient of y_prev (NULL = not wanted).
// All three NULL = the plain entry.
int vrwkv_ln_mix_bwd_carry_bf16(long ntok, int T, int C, int M, const void* xn, const float* mean, const float* rstd, const void* w,
                                const void* b, const void* const* mu, const void* const* dout, const void* dout3_second, const void* dres,
                                const void* y_prev, const float* dy_last, float* dy_prev, void* dx, float* dwb, float* dmu, float* ws,
                                void* stream) {
    return ln_mix_bwd({ntok, T, C, M, xn, mean, rstd, w, b, mu, dout, dout3_second, dres, dx, dwb, dmu, ws, stream, nullptr, y_prev, dy_last, dy_prev});
}

// Modality-routed channel mix (a Block with ln_v / ffn_v for image tokens, VisualRWKV-v7/v7.10/src/model.py:233-262): every row goes through ONE
// of two experts, sel[n] == 0 -> (w[0], b[0], mu[0]) (text: ln2, ffn.x_k), else -> (w[1], b[1], mu[1]) (image: ln_v, ffn_v.x_k).  xn, mean and rstd
// stay in token order; out[pos[n]] = y + (y_prev - y) mu_e with y = LN_e(xn[n]), y_prev = LN_e(xn[n-1]) under row n's expert e (zeros where
// n % T == 0 or first[n] != 0).  pos: ntok int32 (pos_bytes 4) or int64 (8), a permutation of 0 .. ntok-1; first may be NULL.
int vrwkv_ln_mix_routed_fwd_bf16(long ntok, int T, int C, float eps, const void* x, const void* delta, const void* const* w, const void* const* b,
                                 const void* const* mu, void* xn, void* out, float* mean, float* rstd, const unsigned char* first,
                                 const unsigned char* sel, const void* pos, int pos_bytes, void* stream) {
    if (!w || !b || !mu || (pos_bytes != 4 && pos_bytes != 8)) return VRWKV_EINVAL;      // read here; what they hold is the launcher's to check
    const LmRoute rt{(const uint16_t*)w[1], (const uint16_t*)b[1], (const uint16_t*)mu[1], sel, pos, pos_bytes == 8};
    return ln_mix_fwd({ntok, T, C, eps, 1, x, delta, w[0], b[0], mu, xn, &out, mean, rstd, stream, first, nullptr, nullptr, &rt});
}

// its backward: dout (ntok, C) in pos order; dx (ntok, C) in token order = dres + LN'(..) with the row's shared statistics; dwb (2, 2, C) fp32 =
// (dgamma, dbeta) of expert 0, then of expert 1; dmu (2, C) fp32; all written, not accumulated (an expert without rows gets zeros).
// ws: vrwkv_ln_mix_routed_ws_floats(ntok, C) floats.  Deterministic: per-workgroup partial rows summed in a fixed order.
long vrwkv_ln_mix_routed_ws_floats(long ntok, int C) { return (long)ln_mix_bwd_grid(ntok) * 6 * C; }

int vrwkv_ln_mix_routed_bwd_bf16(long ntok, int T, int C, const void* xn, const float* mean, const float* rstd, const void* const* w,
                                 const void* const* b, const void* const* mu, const void* dout, const void* dres, const unsigned char* first,
                                 const unsigned char* sel, const void* pos, int pos_bytes, void* dx, float* dwb, float* dmu, float* ws,
                                 void* stream) {
    if (!w || !b || !mu || (pos_bytes != 4 && pos_bytes != 8)) return VRWKV_EINVAL;      // as in the forward
    const LmRoute rt{(const uint16_t*)w[1], (const uint16_t*)b[1], (const uint16_t*)mu[1], sel, pos, pos_bytes == 8};
    return ln_mix_bwd({ntok, T, C, 1, xn, mean, rstd, w[0], b[0], mu, &dout, nullptr, dres, dx, dwb, dmu, ws, stream, first, nullptr, nullptr, nullptr, &rt});
}

// dst[i] = src[idx[i]] for i < n on rows of C bf16 (C % 8 == 0); idx: n int32 (idx_bytes 4) or int64 (8) on the device, every entry a row of src
int vrwkv_row_gather_bf16(long n, int C, const void* src, const void* idx, int idx_bytes, void* dst, void* stream) {
    if (n <= 0 || !src || !idx || !dst || (idx_bytes != 4 && idx_bytes != 8)) return VRWKV_EINVAL;
    if (C <= 0 || C % 8 != 0) return VRWKV_ESHAPE;
    const long nvec = n * (C / 8);
    const long g = (nvec + 255) / 256;
    const dim3 grid((unsigned)(g > (1L << 20) ? (1L << 20) : g)), block(256);
    if (idx_bytes == 8) hipLaunchKernelGGL(row_gather_kernel<true>, grid, block, 0, (hipStream_t)stream, nvec, C / 8, (const uint16_t*)src, idx, (uint16_t*)dst);
    else hipLaunchKernelGGL(row_gather_kernel<false>, grid, block, 0, (hipStream_t)stream, nvec, C / 8, (const uint16_t*)src, idx, (uint16_t*)dst);
    return finish_launch();
}

}  // extern "C"
