// Kernels of csrc/ln_fused.hip (residual add + LayerNorm, and the same fused with the token shift + lerps of the time-mix /
// channel-mix): kept in a header so that the host lockstep emulator (tests/emu) can run them on the CPU.  See ln_fused.hip for
// the math, the byte counts and the C entry points.
#pragma once
#include <gfx950_prims.h>

namespace vln {

struct V8 { float f[8]; };
DEVFN V8 unpack8(uint4 u) {
    V8 r;
    r.f[0] = bf16_lo(u.x); r.f[1] = bf16_hi(u.x); r.f[2] = bf16_lo(u.y); r.f[3] = bf16_hi(u.y);
    r.f[4] = bf16_lo(u.z); r.f[5] = bf16_hi(u.z); r.f[6] = bf16_lo(u.w); r.f[7] = bf16_hi(u.w);
    return r;
}
DEVFN uint4 pack8(const V8& v) {
    return make_uint4(cvt_pk_bf16(v.f[0], v.f[1]), cvt_pk_bf16(v.f[2], v.f[3]), cvt_pk_bf16(v.f[4], v.f[5]), cvt_pk_bf16(v.f[6], v.f[7]));
}
// Row pieces are streamed: every activation row is read once and written once per kernel, and the tensors (172 MB and more) do not
// survive in L2 / MALL until their consumer runs -- non-temporal accesses (measured per kernel in profiles/r4_eltwise_micro_ab.jsonl)
#ifndef VRWKV_NT
#define VRWKV_NT 1
#endif
typedef uint32_t u32x4_nt __attribute__((ext_vector_type(4)));
DEVFN uint4 ldg(const uint16_t* p) {
#if VRWKV_NT
    const u32x4_nt u = __builtin_nontemporal_load(reinterpret_cast<const u32x4_nt*>(p));
    return make_uint4(u[0], u[1], u[2], u[3]);
#else
    return *reinterpret_cast<const uint4*>(p);
#endif
}
DEVFN void stg(uint16_t* p, uint4 v) {
#if VRWKV_NT
    const u32x4_nt u = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(u, reinterpret_cast<u32x4_nt*>(p));
#else
    *reinterpret_cast<uint4*>(p) = v;
#endif
}
// empty asm that "redefines" a packed loop-invariant row: keeps the compiler from hoisting its unpacked form (twice the registers)
// out of the token loop
DEVFN void keep_packed(uint4& u) { pin_vgpr4(u.x, u.y, u.z, u.w); }

constexpr int MAXW = 16;          // waves per workgroup (C <= 8192)

// all-reduce of NV values over the workgroup; `slot` alternates between consecutive calls
template <int NV>
DEVFN void block_sum(float (*red)[MAXW][2], int slot, int wave, int lane, int nw, float* v) {
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = group_sum<6>(v[i]);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) red[slot][wave][i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = 0.f;
    for (int w = 0; w < nw; ++w) {
#pragma unroll
        for (int i = 0; i < NV; ++i) v[i] += red[slot][w][i];
    }
}

__global__ __launch_bounds__(1024) void add_ln_fwd_kernel(long ntok, int C, float eps, const uint16_t* __restrict__ x,
                                                          const uint16_t* __restrict__ delta, const uint16_t* __restrict__ w,
                                                          const uint16_t* __restrict__ b, uint16_t* __restrict__ xn,
                                                          uint16_t* __restrict__ y, float* __restrict__ mean, float* __restrict__ rstd,
                                                          const long* __restrict__ yrow, const uint16_t* __restrict__ dscale = nullptr) {
    __shared__ float red[4][MAXW][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int c0 = threadIdx.x * 8;
    const bool act = c0 < C;
    const long lo = ntok * blockIdx.x / gridDim.x, hi = ntok * (blockIdx.x + 1) / gridDim.x;
    if (lo >= hi) return;
    const uint4 z4 = make_uint4(0, 0, 0, 0);
    const V8 wv = unpack8(act ? ldg(w + c0) : z4), bv = unpack8(act ? ldg(b + c0) : z4);
    const V8 sv = unpack8((act && dscale) ? ldg(dscale + c0) : z4);         // optional per-channel scale of delta (ViT LayerScale)
    const float inv_c = 1.f / (float)C;
    uint4 nx = act ? ldg(x + lo * C + c0) : z4, nd = (act && delta) ? ldg(delta + lo * C + c0) : z4;
    for (long n = lo; n < hi; ++n) {
        const uint4 cx = nx, cd = nd;
        if (n + 1 < hi && act) {
            nx = ldg(x + (n + 1) * C + c0);
            if (delta) nd = ldg(delta + (n + 1) * C + c0);
        }
        V8 v = unpack8(cx);
        if (delta) {
            const V8 d = unpack8(cd);
            if (dscale) {
#pragma unroll
                for (int e = 0; e < 8; ++e) v.f[e] = fmaf(d.f[e], sv.f[e], v.f[e]);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) v.f[e] += d.f[e];
            }
            const uint4 r = pack8(v);
            if (act) stg(xn + n * C + c0, r);
            v = unpack8(r);
        }
        const int par = (int)(n & 1) * 2;
        float s[1] = {0.f};
#pragma unroll
        for (int e = 0; e < 8; ++e) s[0] += v.f[e];
        block_sum<1>(red, par, wave, lane, nw, s);
        const float mu = s[0] * inv_c;
        float q[1] = {0.f};
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float t = act ? v.f[e] - mu : 0.f; q[0] = fmaf(t, t, q[0]); }
        block_sum<1>(red, par + 1, wave, lane, nw, q);
        const float rs = rsqrtf(q[0] * inv_c + eps);
        V8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o.f[e] = fmaf((v.f[e] - mu) * rs, wv.f[e], bv.f[e]);
        const long orow = yrow ? yrow[n] : n;                  // yrow: scatter into a larger tensor; a negative row is dropped
        if (act && orow >= 0) stg(y + orow * C + c0, pack8(o));
        if (threadIdx.x == 0 && mean) { mean[n] = mu; rstd[n] = rs; }
    }
}

__global__ __launch_bounds__(1024) void add_ln_bwd_kernel(long ntok, int C, const uint16_t* __restrict__ dy,
                                                          const uint16_t* __restrict__ dres, const uint16_t* __restrict__ xn,
                                                          const float* __restrict__ mean, const float* __restrict__ rstd,
                                                          const uint16_t* __restrict__ w, uint16_t* __restrict__ dx,
                                                          float* __restrict__ part, const long* __restrict__ yrow) {
    __shared__ float red[2][MAXW][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int c0 = threadIdx.x * 8;
    const bool act = c0 < C;
    const long lo = ntok * blockIdx.x / gridDim.x, hi = ntok * (blockIdx.x + 1) / gridDim.x;
    const uint4 z4 = make_uint4(0, 0, 0, 0);
    const V8 wv = unpack8(act ? ldg(w + c0) : z4);
    const float inv_c = 1.f / (float)C;
    V8 gw, gb;
#pragma unroll
    for (int e = 0; e < 8; ++e) { gw.f[e] = 0.f; gb.f[e] = 0.f; }
    uint4 ny = z4, nx = z4, nr = z4;
    float nmu = 0.f, nrs = 0.f;
    if (lo < hi) {
        if (act) { const long r = yrow ? yrow[lo] : lo; ny = r >= 0 ? ldg(dy + r * C + c0) : z4; nx = ldg(xn + lo * C + c0); if (dres) nr = ldg(dres + lo * C + c0); }
        nmu = mean[lo]; nrs = rstd[lo];
    }
    for (long n = lo; n < hi; ++n) {
        const uint4 cy = ny, cx = nx, cr = nr;
        const float mu = nmu, rs = nrs;
        if (n + 1 < hi) {
            if (act) { const long r = yrow ? yrow[n + 1] : n + 1; ny = r >= 0 ? ldg(dy + r * C + c0) : z4; nx = ldg(xn + (n + 1) * C + c0); if (dres) nr = ldg(dres + (n + 1) * C + c0); }
            nmu = mean[n + 1]; nrs = rstd[n + 1];
        }
        const V8 d = unpack8(cy), xv = unpack8(cx);
        V8 xh, g;
        float s[2] = {0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            xh.f[e] = act ? (xv.f[e] - mu) * rs : 0.f;
            g.f[e] = d.f[e] * wv.f[e];
            s[0] += g.f[e];
            s[1] = fmaf(g.f[e], xh.f[e], s[1]);
            gw.f[e] = fmaf(d.f[e], xh.f[e], gw.f[e]);
            gb.f[e] += d.f[e];
        }
        block_sum<2>(red, (int)(n & 1), wave, lane, nw, s);
        const float c1 = s[0] * inv_c, c2 = s[1] * inv_c;
        V8 o = unpack8(cr);                         // zeros when there is no residual gradient
#pragma unroll
        for (int e = 0; e < 8; ++e) o.f[e] = fmaf(rs, g.f[e] - c1 - xh.f[e] * c2, o.f[e]);
        if (act) stg(dx + n * C + c0, pack8(o));
    }
    if (act) {
        float* dst = part + (size_t)blockIdx.x * 2 * C + c0;
        *reinterpret_cast<float4*>(dst) = make_float4(gw.f[0], gw.f[1], gw.f[2], gw.f[3]);
        *reinterpret_cast<float4*>(dst + 4) = make_float4(gw.f[4], gw.f[5], gw.f[6], gw.f[7]);
        *reinterpret_cast<float4*>(dst + C) = make_float4(gb.f[0], gb.f[1], gb.f[2], gb.f[3]);
        *reinterpret_cast<float4*>(dst + C + 4) = make_float4(gb.f[4], gb.f[5], gb.f[6], gb.f[7]);
    }
}

// out[j] = sum_g part[g][j], fixed order (same scheme as tmix_fused.hip's colsum_kernel); width % 16 == 0
__global__ __launch_bounds__(256) void ln_colsum_kernel(int G, long width, const float* __restrict__ part, float* __restrict__ out) {
    // A workgroup owns 16 columns; thread (cq = tid & 3, rg = tid >> 2) sums rows rg, rg+64, ... of 4 adjacent columns (float4); the 64
    // row groups are combined through LDS in a fixed order (deterministic).  (64 columns per workgroup left half of the CUs without
    // work for the 2-8 k columns of a parameter gradient: 23 / 46 us per call, 5 ms per training step.)
    __shared__ float4 red[64][4];
    __shared__ float4 red2[8][4];
    const int cq = threadIdx.x & 3, rg = threadIdx.x >> 2;
    const long col = (long)blockIdx.x * 16 + 4 * cq;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int g = rg; g < G; g += 64) {
        const float4 v = *reinterpret_cast<const float4*>(part + (size_t)g * width + col);
        a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
    red[rg][cq] = a;
    __syncthreads();
    if (rg < 8) {
        float4 t = red[rg][cq];
#pragma unroll
        for (int r = rg + 8; r < 64; r += 8) { const float4 v = red[r][cq]; t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w; }
        red2[rg][cq] = t;
    }
    __syncthreads();
    if (rg == 0) {
        float4 t = red2[0][cq];
#pragma unroll
        for (int r = 1; r < 8; ++r) { const float4 v = red2[r][cq]; t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w; }
        *reinterpret_cast<float4*>(out + col) = t;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// Residual add + LayerNorm + token shift + M lerps in one pass (Block: x = x + att(ln1(x)) with RWKV_Tmix_x070's six lerps,
// x = x + ffn(ln2(x)) with RWKV_CMix_x070's one: VisualRWKV-v7/v7.00/src/model.py:247-254,166-173,222-223).  The LayerNorm output is
// used by nothing but the lerps, so it is never written: forward 4 B/element less than add_ln + mix (8 + 14 -> 18 for M = 6,
// 8 + 4 -> 8 for M = 1), backward 6 B/element less (16 + 8 -> 18, 6 + 8 -> 8), and one saved activation less per LayerNorm.
// Same arithmetic as the two-kernel path, rounding included (the LayerNorm output and the lerps' input gradient are rounded to
// bf16 where that path stores them), so outputs and input gradients are bit-identical to it.
//   forward : xn = bf16(x + delta);  y = bf16(LN(xn));  out_j[n] = y[n] + (y[n-1] - y[n]) mu_j   (y[-1] = 0 at the start of a sample)
//   backward: dyl[n] = bf16(A[n] + Bv[n+1]),  A = sum_j d_j (1 - mu_j),  Bv = sum_j d_j mu_j;  dx = dres + LN'(dyl);
//             dmu_j = sum_n d_j[n] (y[n-1] - y[n]),  dw, db as in add_ln_bwd;  y is recomputed from xn and the saved statistics.
// A workgroup walks a contiguous token range in order (the row before the range is recomputed / the row after it read once).
struct LmPtrs { const uint16_t* p[6]; };
struct LmOuts { uint16_t* p[6]; };

// PK (the _packed entries: rows that hold several samples end to end): first_tok[n] != 0 marks the first token of a sample next to n % T == 0;
// one byte per 2 C-byte row, read once per row at a wave-uniform address.  With PK off the pointer is never read.
// CARRY (the _carry entries: a row cut into segments that are trained one after the other): y_prev (B, C) bf16 = the LayerNorm output of the row
// before each sample's first row, in place of the zeros at n % T == 0; y_last (B, C) bf16 receives the LayerNorm output of each sample's last
// row (what `prev` holds after it).  Either may be NULL; with CARRY off neither is read.
// ROUTED (the _routed entries, M = 1: a Block with a second LayerNorm + channel mix for image tokens, VisualRWKV-v7/v7.10/src/model.py:233-262):
// sel[n] != 0 sends row n through expert 1 = (w1, b1, mu1), else through expert 0 = the kernel's own (w, b, mu.p[0]).  The statistics of a row
// belong to xn alone; its lerp reads the row before under ITS expert, LN_e(n)(xn[n-1]), whatever expert that row went through itself.
// pos[n] (int32, or int64 with pos64) is the row of token n in the routed tensor: where the forward writes out, where the backward reads dout.
// One byte of sel (and of first_tok) per 2 C-byte row, at a wave-uniform address: read as a scalar.  With ROUTED off nothing of this is read.
struct LmRoute {
    const uint16_t *w1, *b1, *mu1;
    const unsigned char* sel;
    const void* pos;
    int pos64;
};
// wkv7::uniform_flag_u8 (wkv7_kernels.h) with a 64-bit index; repeated here because the emulator compiles this header inside a namespace of its own
DEVFN unsigned uniform_flag_u8(const unsigned char* flags, long idx) {
#if defined(__HIP_DEVICE_COMPILE__)
    const unsigned long long a = (unsigned long long)(uintptr_t)(flags + idx);
    typedef __attribute__((address_space(4))) const unsigned* const_u32_ptr;
    const unsigned word = *(const_u32_ptr)(a & ~3ull);
    return __builtin_amdgcn_readfirstlane((word >> (8u * ((unsigned)a & 3u))) & 0xffu);
#else
    return flags[idx];
#endif
}
DEVFN long route_row(const LmRoute& rt, long n) {
    return rt.pos64 ? reinterpret_cast<const long*>(rt.pos)[n] : (long)reinterpret_cast<const int*>(rt.pos)[n];
}

template <int M, bool PK = false, bool CARRY = false, bool ROUTED = false>
__global__ __launch_bounds__(1024) void ln_mix_fwd_kernel(long ntok, int T, int C, float eps, const uint16_t* __restrict__ x,
                                                          const uint16_t* __restrict__ delta, const uint16_t* __restrict__ w,
                                                          const uint16_t* __restrict__ b, uint16_t* __restrict__ xn,
                                                          float* __restrict__ mean, float* __restrict__ rstd, LmPtrs mu, LmOuts out,
                                                          const unsigned char* __restrict__ first_tok = nullptr,
                                                          const uint16_t* __restrict__ y_prev = nullptr, uint16_t* __restrict__ y_last = nullptr,
                                                          LmRoute rt = LmRoute()) {
    static_assert(!ROUTED || (M == 1 && !CARRY), "ROUTED: the channel-mix lerp of an uncut row");
    __shared__ float red[4][MAXW][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int c0 = threadIdx.x * 8;
    const bool act = c0 < C;
    const long lo = ntok * blockIdx.x / gridDim.x, hi = ntok * (blockIdx.x + 1) / gridDim.x;
    if (lo >= hi) return;
    const uint4 z4 = make_uint4(0, 0, 0, 0);
    const V8 wv = unpack8(act ? ldg(w + c0) : z4), bv = unpack8(act ? ldg(b + c0) : z4);
    uint4 mp[M];                                                 // lerp weights, packed (unpacked where used: registers)
#pragma unroll
    for (int j = 0; j < M; ++j) mp[j] = act ? ldg(mu.p[j] + c0) : z4;
    uint4 w1p = z4, b1p = z4, m1p = z4;                          // ROUTED: expert 1, packed like mp
    if (ROUTED && act) { w1p = ldg(rt.w1 + c0); b1p = ldg(rt.b1 + c0); m1p = ldg(rt.mu1 + c0); }
    const float inv_c = 1.f / (float)C;
    const long n0 = (lo % T != 0) ? lo - 1 : lo;                 // the row before the range: only its LayerNorm output is needed
    uint4 nx = act ? ldg(x + n0 * C + c0) : z4, nd = (act && delta) ? ldg(delta + n0 * C + c0) : z4;
    V8 prev;
#pragma unroll
    for (int e = 0; e < 8; ++e) prev.f[e] = 0.f;
    int tpos = (int)(n0 % T);                                    // position of row n inside its sample (one division per workgroup)
    long samp = CARRY ? n0 / T : 0;                              // CARRY: the sample of row n, counted along (no division per row)
    for (long n = n0; n < hi; ++n) {
        const uint4 cx = nx, cd = nd;
        if (n + 1 < hi && act) {
            nx = ldg(x + (n + 1) * C + c0);
            if (delta) nd = ldg(delta + (n + 1) * C + c0);
        }
        const bool own = n >= lo;
        V8 v = unpack8(cx);
        if (delta) {
            const V8 d = unpack8(cd);
#pragma unroll
            for (int e = 0; e < 8; ++e) v.f[e] += d.f[e];
            const uint4 r = pack8(v);
            if (act && own) stg(xn + n * C + c0, r);
            v = unpack8(r);
        }
        const int par = (int)(n & 1) * 2;
        float s[1] = {0.f};
#pragma unroll
        for (int e = 0; e < 8; ++e) s[0] += v.f[e];
        block_sum<1>(red, par, wave, lane, nw, s);
        const float mu_ = s[0] * inv_c;
        float q[1] = {0.f};
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float t = act ? v.f[e] - mu_ : 0.f; q[0] = fmaf(t, t, q[0]); }
        block_sum<1>(red, par + 1, wave, lane, nw, q);
        const float rs = rsqrtf(q[0] * inv_c + eps);
        if (ROUTED) {
            // `prev` carries the normalised row (v - mean) rstd: the LayerNorm output of the row before is re-formed from it under this row's
            // expert with the operations of the plain kernel, so a row's output has the bits of that kernel run with this expert's parameters
            V8 xh;
#pragma unroll
            for (int e = 0; e < 8; ++e) xh.f[e] = (v.f[e] - mu_) * rs;
            if (own) {
                const bool img = uniform_flag_u8(rt.sel, n) != 0;
                const V8 we = img ? unpack8(w1p) : wv, be = img ? unpack8(b1p) : bv, m = unpack8(img ? m1p : mp[0]);
                const bool first = tpos == 0 || (PK && uniform_flag_u8(first_tok, n) != 0);
                V8 o, op;
#pragma unroll
                for (int e = 0; e < 8; ++e) { o.f[e] = fmaf(xh.f[e], we.f[e], be.f[e]); op.f[e] = fmaf(prev.f[e], we.f[e], be.f[e]); }
                const V8 cur = unpack8(pack8(o)), yp = unpack8(pack8(op));
                V8 r;
#pragma unroll
                for (int e = 0; e < 8; ++e) r.f[e] = fmaf((first ? 0.f : yp.f[e]) - cur.f[e], m.f[e], cur.f[e]);
                if (act) stg(out.p[0] + route_row(rt, n) * C + c0, pack8(r));
                if (threadIdx.x == 0) { mean[n] = mu_; rstd[n] = rs; }
            }
            prev = xh;
            if (++tpos == T) tpos = 0;
            continue;
        }
        V8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o.f[e] = fmaf((v.f[e] - mu_) * rs, wv.f[e], bv.f[e]);
        const V8 cur = unpack8(pack8(o));                        // the bf16 value the two-kernel path stores and re-reads
        if (own) {
            bool first = tpos == 0 || (PK && first_tok[n] != 0);
            if (CARRY && tpos == 0 && y_prev) {                  // the segment before this one ended in this row's predecessor
                prev = unpack8(act ? ldg(y_prev + samp * C + c0) : z4);
                first = false;
            }
            V8 xx;
#pragma unroll
            for (int e = 0; e < 8; ++e) xx.f[e] = (first ? 0.f : prev.f[e]) - cur.f[e];
#pragma unroll
            for (int j = 0; j < M; ++j) {
                const V8 m = unpack8(mp[j]);
                V8 r;
#pragma unroll
                for (int e = 0; e < 8; ++e) r.f[e] = fmaf(xx.f[e], m.f[e], cur.f[e]);
                if (act) stg(out.p[j] + n * C + c0, pack8(r));
            }
            if (threadIdx.x == 0) { mean[n] = mu_; rstd[n] = rs; }
            if (CARRY && y_last && tpos == T - 1 && act) stg(y_last + samp * C + c0, pack8(o));
        }
        prev = cur;
        if (++tpos == T) { tpos = 0; if (CARRY) ++samp; }
    }
}

// LayerNorm backward of one finished row (the body of add_ln_bwd_kernel's loop): dyl = gradient of the LayerNorm output (already
// rounded to bf16), xh / rs of that row, res = the residual path's gradient (packed; zeros: none)
DEVFN void ln_row_bwd(float (*red)[MAXW][2], int slot, int wave, int lane, int nw, bool act, float inv_c, const V8& wv, const V8& dyl,
                      const V8& xh, float rs, uint4 res, V8& gw, V8& gb, uint16_t* dst) {
    V8 g;
    float s[2] = {0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        g.f[e] = dyl.f[e] * wv.f[e];
        s[0] += g.f[e];
        s[1] = fmaf(g.f[e], xh.f[e], s[1]);
        gw.f[e] = fmaf(dyl.f[e], xh.f[e], gw.f[e]);
        gb.f[e] += dyl.f[e];
    }
    block_sum<2>(red, slot, wave, lane, nw, s);
    const float c1 = s[0] * inv_c, c2 = s[1] * inv_c;
    V8 o = unpack8(res);
#pragma unroll
    for (int e = 0; e < 8; ++e) o.f[e] = fmaf(rs, g.f[e] - c1 - xh.f[e] * c2, o.f[e]);
    if (act) stg(dst, pack8(o));
}

// The ROUTED form of ln_mix_bwd_kernel (M = 1).  Row n's lerp went through expert e(n), so the gradient of the normalised row n collects
//   w_e(n) dout[n] (1 - mu_e(n))  +  w_e(n+1) dout[n+1] mu_e(n+1)       (the second term: row n+1 read row n under ITS expert)
// and one LayerNorm backward follows with the row's statistics, which both experts share.  Where e(n) == e(n+1) the two terms are added
// before the bf16 rounding and the row takes the plain kernel's path, operation for operation; where they differ each term is rounded on
// its own (two LayerNorm outputs, two gradients) and dw / db take each from the expert it came through.
// Registers hold the parameters and the partial sums (dw, db, dmu) of ONE expert, the current row's: a workgroup walks its rows in order and
// an expert change is rare on real rows (one image block per sample).  At a change the sums go to the workgroup's own partial row of that
// expert (plain vector stores) and the other expert's are taken up again from there, or from zero: one writer per address, a fixed order.
template <bool PK>
DEVFN void ln_mix_bwd_routed(float (*red)[MAXW][2], long ntok, int T, int C, const uint16_t* __restrict__ xn, const float* __restrict__ mean,
                             const float* __restrict__ rstd, const uint16_t* __restrict__ w0, const uint16_t* __restrict__ b0,
                             const uint16_t* __restrict__ mu0, const uint16_t* __restrict__ dout, const uint16_t* __restrict__ dres,
                             uint16_t* __restrict__ dx, float* __restrict__ part_ln, float* __restrict__ part_mu,
                             const unsigned char* __restrict__ first_tok, const LmRoute& rt) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int c0 = threadIdx.x * 8;
    const bool act = c0 < C;
    const long lo = ntok * blockIdx.x / gridDim.x, hi = ntok * (blockIdx.x + 1) / gridDim.x;
    const uint4 z4 = make_uint4(0, 0, 0, 0);
    const int cc = act ? c0 : 0;
    const float inv_c = 1.f / (float)C;
    float* pl = part_ln + (size_t)blockIdx.x * 4 * C + cc;       // [expert][dw | db][C]
    float* pm = part_mu + (size_t)blockIdx.x * 2 * C + cc;       // [expert][C]
    V8 gw, gb, gm;
#pragma unroll
    for (int e = 0; e < 8; ++e) { gw.f[e] = 0.f; gb.f[e] = 0.f; gm.f[e] = 0.f; }
    auto st8 = [&](float* p, const V8& v) {
        *reinterpret_cast<float4*>(p) = make_float4(v.f[0], v.f[1], v.f[2], v.f[3]);
        *reinterpret_cast<float4*>(p + 4) = make_float4(v.f[4], v.f[5], v.f[6], v.f[7]);
    };
    auto ld8 = [&](const float* p) {
        const float4 a = *reinterpret_cast<const float4*>(p), c = *reinterpret_cast<const float4*>(p + 4);
        V8 r;
        r.f[0] = a.x; r.f[1] = a.y; r.f[2] = a.z; r.f[3] = a.w; r.f[4] = c.x; r.f[5] = c.y; r.f[6] = c.z; r.f[7] = c.w;
        return r;
    };
    auto put_sums = [&](int ex) {
        if (act) { st8(pl + (size_t)ex * 2 * C, gw); st8(pl + (size_t)ex * 2 * C + C, gb); st8(pm + (size_t)ex * C, gm); }
    };
    unsigned stored = 0;                                         // wave-uniform, bit e: has expert e's partial row been written?
    int ex = 0;
    if (lo < hi) {
        ex = uniform_flag_u8(rt.sel, lo) != 0;
        uint4 wp = z4, bp = z4, mp = z4;
        auto load_params = [&](int e) {
            if (act) { wp = ldg((e ? rt.w1 : w0) + c0); bp = ldg((e ? rt.b1 : b0) + c0); mp = ldg((e ? rt.mu1 : mu0) + c0); }
        };
        load_params(ex);
        auto ln_out = [&](uint4 xp, float m0, float r0) {
            const V8 xv = unpack8(xp), wv = unpack8(wp), bv = unpack8(bp);
            V8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o.f[e] = fmaf((xv.f[e] - m0) * r0, wv.f[e], bv.f[e]);
            return unpack8(pack8(o));
        };
        V8 aprev;
#pragma unroll
        for (int e = 0; e < 8; ++e) aprev.f[e] = 0.f;
        uint4 xprev = z4, resprev = z4;
        float muprev = 0.f, rsprev = 0.f;
        if (lo % T != 0) { xprev = ldg(xn + (lo - 1) * C + cc); muprev = mean[lo - 1]; rsprev = rstd[lo - 1]; }
        const long last = (hi < ntok && hi % T != 0) ? hi : hi - 1;
        uint4 nd, nx, nr = z4;
        float nmu, nrs;
        nd = ldg(dout + route_row(rt, lo) * C + cc);
        nx = ldg(xn + lo * C + cc);
        if (dres) nr = ldg(dres + lo * C + cc);
        nmu = mean[lo]; nrs = rstd[lo];
        int slot = 0;
        int tpos = (int)(lo % T);
        for (long n = lo; n <= last; ++n) {
            const bool inside = n < hi, cont = tpos != 0 && !(PK && uniform_flag_u8(first_tok, n) != 0);
            const int en = uniform_flag_u8(rt.sel, n) != 0;
            const bool cross = en != ex;                         // n > lo: ex is the expert of row n-1
            V8 ga = aprev;                                       // (only read after a change of expert)
            if (cross) {
                // row n-1's own term leaves through the expert it came through, whose parameters and sums are still in the registers
                const V8 xv = unpack8(xprev), wv = unpack8(wp), t = unpack8(pack8(aprev));
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float xh = act ? (xv.f[e] - muprev) * rsprev : 0.f;
                    ga.f[e] = t.f[e] * wv.f[e];
                    gw.f[e] = fmaf(t.f[e], xh, gw.f[e]);
                    gb.f[e] += t.f[e];
                }
                put_sums(ex);
                stored |= 1u << ex;
                ex = en;
                load_params(ex);
                if ((stored >> ex) & 1u) { gw = ld8(pl + (size_t)ex * 2 * C); gb = ld8(pl + (size_t)ex * 2 * C + C); gm = ld8(pm + (size_t)ex * C); }
                else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) { gw.f[e] = 0.f; gb.f[e] = 0.f; gm.f[e] = 0.f; }
                }
            }
            keep_packed(wp); keep_packed(bp); keep_packed(mp);
            const uint4 cx = nx, cr = nr;
            const float mu_ = nmu, rs = nrs;
            V8 xx;
            {
                const V8 y = ln_out(cx, mu_, rs), yp = ln_out(xprev, muprev, rsprev);
#pragma unroll
                for (int e = 0; e < 8; ++e) xx.f[e] = inside ? (cont ? yp.f[e] : 0.f) - y.f[e] : 0.f;
            }
            V8 dsum, bvv;
            {
                const V8 d = unpack8(nd), m = unpack8(mp);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    dsum.f[e] = 0.f + d.f[e];
                    bvv.f[e] = fmaf(d.f[e], m.f[e], 0.f);
                    gm.f[e] = fmaf(d.f[e], xx.f[e], gm.f[e]);
                }
            }
            if (n + 1 <= last) {
                const long o = (n + 1) * C + cc;
                nd = ldg(dout + route_row(rt, n + 1) * C + cc);
                if (n + 1 < hi) {
                    nx = ldg(xn + o);
                    if (dres) nr = ldg(dres + o);
                    nmu = mean[n + 1]; nrs = rstd[n + 1];
                }
            }
            if (n > lo) {
                V8 xh;
                const V8 xv = unpack8(xprev);
#pragma unroll
                for (int e = 0; e < 8; ++e) xh.f[e] = act ? (xv.f[e] - muprev) * rsprev : 0.f;
                if (!cross) {                                    // one expert on both sides: the plain kernel's row
                    V8 t;
#pragma unroll
                    for (int e = 0; e < 8; ++e) t.f[e] = aprev.f[e] + (cont ? bvv.f[e] : 0.f);
                    ln_row_bwd(red, slot, wave, lane, nw, act, inv_c, unpack8(wp), unpack8(pack8(t)), xh, rsprev, resprev, gw, gb, dx + (n - 1) * C + cc);
                } else {                                         // ga = row n-1's own term times its expert's w; row n's term comes through this expert
                    const V8 wv = unpack8(wp), tb = unpack8(pack8(bvv));
                    V8 g;
                    float s[2] = {0.f, 0.f};
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float t = cont ? tb.f[e] : 0.f;
                        g.f[e] = fmaf(t, wv.f[e], ga.f[e]);
                        s[0] += g.f[e];
                        s[1] = fmaf(g.f[e], xh.f[e], s[1]);
                        gw.f[e] = fmaf(t, xh.f[e], gw.f[e]);
                        gb.f[e] += t;
                    }
                    block_sum<2>(red, slot, wave, lane, nw, s);
                    const float c1 = s[0] * inv_c, c2 = s[1] * inv_c;
                    V8 o = unpack8(resprev);
#pragma unroll
                    for (int e = 0; e < 8; ++e) o.f[e] = fmaf(rsprev, g.f[e] - c1 - xh.f[e] * c2, o.f[e]);
                    if (act) stg(dx + (n - 1) * C + cc, pack8(o));
                }
                slot ^= 1;
            }
            if (inside) {
#pragma unroll
                for (int e = 0; e < 8; ++e) aprev.f[e] = dsum.f[e] - bvv.f[e];
                xprev = cx; resprev = cr; muprev = mu_; rsprev = rs;
            }
            if (++tpos == T) tpos = 0;
        }
        if (last == hi - 1) {                                    // no successor row: the gradient of the last row is A
            V8 xh;
            const V8 xv = unpack8(xprev);
#pragma unroll
            for (int e = 0; e < 8; ++e) xh.f[e] = act ? (xv.f[e] - muprev) * rsprev : 0.f;
            ln_row_bwd(red, slot, wave, lane, nw, act, inv_c, unpack8(wp), unpack8(pack8(aprev)), xh, rsprev, resprev, gw, gb, dx + (hi - 1) * C + cc);
        }
    }
    put_sums(ex);
    if (!((stored >> (ex ^ 1)) & 1u)) {                                       // an expert without a row in this range: zeros
#pragma unroll
        for (int e = 0; e < 8; ++e) { gw.f[e] = 0.f; gb.f[e] = 0.f; gm.f[e] = 0.f; }
        put_sums(ex ^ 1);
    }
}


// DUP3: output 3 (x_v) has two consumers; their gradients arrive as dout.p[3] and dout3b (see mix_bwd_kernel in tmix_fused.hip).
// LB: threads per workgroup the instantiation is compiled for (C / 8 rounded up to a wave).  Register discipline (M = 6 keeps 48
// gradient accumulators per thread): rows travel packed (bf16) and are unpacked where used, the previous row is carried as packed
// xn + its two statistics and its LayerNorm output is recomputed, and the next row's loads are issued after this row's values
// have been consumed and before the reduction -- the kernel needs ~2 us of HBM time per row and CU, the arithmetic ~0.3.
// CARRY (the _carry entries): y_prev as in the forward; dy_last (B, C) fp32 = the gradient that reaches the LayerNorm output of each sample's
// last row from the segment after it, added to that row's A in place of a continuing row's Bv; dy_prev (B, C) fp32 receives Bv of each sample's first
// row, the term that has nowhere to go without a carry.  fp32 both: aprev + Bv is formed in fp32 and rounded once.  Each may be NULL.
// ROUTED: see ln_mix_bwd_routed above; dout.p[0] is then in routed row order (rt.pos), part_ln holds (2, 2, C) and part_mu (2, C) per workgroup.
template <int M, bool DUP3, int LB, bool PK = false, bool CARRY = false, bool ROUTED = false>
__global__ __launch_bounds__(LB, LB <= 256 ? 2 : 1) void ln_mix_bwd_kernel(long ntok, int T, int C, const uint16_t* __restrict__ xn,
                                                        const float* __restrict__ mean, const float* __restrict__ rstd,
                                                        const uint16_t* __restrict__ w, const uint16_t* __restrict__ b, LmPtrs mu,
                                                        LmPtrs dout, const uint16_t* __restrict__ dout3b,
                                                        const uint16_t* __restrict__ dres, uint16_t* __restrict__ dx,
                                                        float* __restrict__ part_ln, float* __restrict__ part_mu,
                                                        const unsigned char* __restrict__ first_tok = nullptr,
                                                        const uint16_t* __restrict__ y_prev = nullptr, const float* __restrict__ dy_last = nullptr,
                                                        float* __restrict__ dy_prev = nullptr, LmRoute rt = LmRoute()) {
    static_assert(!ROUTED || (M == 1 && !DUP3 && !CARRY), "ROUTED: the channel-mix lerp of an uncut row");
    __shared__ float red[2][MAXW][2];
    if (ROUTED) {
        ln_mix_bwd_routed<PK>(red, ntok, T, C, xn, mean, rstd, w, b, mu.p[0], dout.p[0], dres, dx, part_ln, part_mu, first_tok, rt);
        return;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int c0 = threadIdx.x * 8;
    const bool act = c0 < C;
    const long lo = ntok * blockIdx.x / gridDim.x, hi = ntok * (blockIdx.x + 1) / gridDim.x;
    const uint4 z4 = make_uint4(0, 0, 0, 0);
    const int cc = act ? c0 : 0;                                 // inactive lanes (C / 8 not a multiple of 64) read column 0, store nothing
    uint4 wp = act ? ldg(w + c0) : z4, bp = act ? ldg(b + c0) : z4;
    uint4 mp[M];
#pragma unroll
    for (int j = 0; j < M; ++j) mp[j] = act ? ldg(mu.p[j] + c0) : z4;
    const float inv_c = 1.f / (float)C;
    V8 gw, gb, gm[M];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        gw.f[e] = 0.f; gb.f[e] = 0.f;
#pragma unroll
        for (int j = 0; j < M; ++j) gm[j].f[e] = 0.f;
    }
    // LayerNorm output of a row as the forward rounded it, from its packed xn and statistics
    auto ln_out = [&](uint4 xp, float m0, float r0) {
        const V8 xv = unpack8(xp), wv = unpack8(wp), bv = unpack8(bp);
        V8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o.f[e] = fmaf((xv.f[e] - m0) * r0, wv.f[e], bv.f[e]);
        return unpack8(pack8(o));
    };
    // CARRY: 8 floats of a (B, C) fp32 carry row; inactive lanes read column 0 like every other load here
    auto ld8 = [&](const float* p) {
        const float4 a = *reinterpret_cast<const float4*>(p), c = *reinterpret_cast<const float4*>(p + 4);
        V8 r;
        r.f[0] = a.x; r.f[1] = a.y; r.f[2] = a.z; r.f[3] = a.w; r.f[4] = c.x; r.f[5] = c.y; r.f[6] = c.z; r.f[7] = c.w;
        return r;
    };
    if (lo < hi) {
        V8 aprev;
#pragma unroll
        for (int e = 0; e < 8; ++e) aprev.f[e] = 0.f;
        uint4 xprev = z4, resprev = z4;                          // previous row: packed xn, residual gradient, statistics
        float muprev = 0.f, rsprev = 0.f;
        if (lo % T != 0) { xprev = ldg(xn + (lo - 1) * C + cc); muprev = mean[lo - 1]; rsprev = rstd[lo - 1]; }
        // rows lo .. hi-1 in full; row hi (if it continues the last sequence) contributes only Bv to the gradient of row hi-1
        const long last = (hi < ntok && hi % T != 0) ? hi : hi - 1;
        uint4 nd[M], nd3 = z4, nx, nr = z4;
        float nmu, nrs;
#pragma unroll
        for (int j = 0; j < M; ++j) nd[j] = ldg(dout.p[j] + lo * C + cc);
        if (DUP3) nd3 = ldg(dout3b + lo * C + cc);
        nx = ldg(xn + lo * C + cc);
        if (dres) nr = ldg(dres + lo * C + cc);
        nmu = mean[lo]; nrs = rstd[lo];
        int slot = 0;
        int tpos = (int)(lo % T);                                // position of row n inside its sample
        long samp = CARRY ? lo / T : 0;                          // CARRY: the sample of row n, counted along (no division per row)
        for (long n = lo; n <= last; ++n) {
            const bool inside = n < hi, cont = tpos != 0 && !(PK && first_tok[n] != 0);      // PK: nothing goes from a sample's first row to the row before
            keep_packed(wp); keep_packed(bp);
#pragma unroll
            for (int j = 0; j < M; ++j) keep_packed(mp[j]);
            const uint4 cx = nx, cr = nr;
            const float mu_ = nmu, rs = nrs;
            // shift difference of the lerps at this row: y[n-1] - y[n]
            V8 xx;
            {
                const V8 y = ln_out(cx, mu_, rs);
                const bool carried = CARRY && tpos == 0 && y_prev;          // the row before is the last one of the segment before
                V8 yp;
                if (carried) yp = unpack8(ldg(y_prev + samp * C + cc));
                else yp = ln_out(xprev, muprev, rsprev);
                const bool shifted = cont || carried;
#pragma unroll
                for (int e = 0; e < 8; ++e) xx.f[e] = inside ? (shifted ? yp.f[e] : 0.f) - y.f[e] : 0.f;
            }
            V8 dsum, bvv;
#pragma unroll
            for (int e = 0; e < 8; ++e) { dsum.f[e] = 0.f; bvv.f[e] = 0.f; }
#pragma unroll
            for (int j = 0; j < M; ++j) {
                V8 d = unpack8(nd[j]);
                if (DUP3 && j == (M > 3 ? 3 : 0)) {
                    const V8 d2 = unpack8(nd3);
#pragma unroll
                    for (int e = 0; e < 8; ++e) d.f[e] += d2.f[e];
                }
                const V8 m = unpack8(mp[j]);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    dsum.f[e] += d.f[e];
                    bvv.f[e] = fmaf(d.f[e], m.f[e], bvv.f[e]);
                    gm[j].f[e] = fmaf(d.f[e], xx.f[e], gm[j].f[e]);
                }
            }
            if (CARRY && dy_prev && tpos == 0 && inside && act) {   // Bv of a sample's first row: the gradient of y_prev
                float* dp = dy_prev + samp * C + c0;
                *reinterpret_cast<float4*>(dp) = make_float4(bvv.f[0], bvv.f[1], bvv.f[2], bvv.f[3]);
                *reinterpret_cast<float4*>(dp + 4) = make_float4(bvv.f[4], bvv.f[5], bvv.f[6], bvv.f[7]);
            }
            if (n + 1 <= last) {                                 // next row's loads: this row's registers are free, the reduction is ahead
                const long o = (n + 1) * C + cc;
#pragma unroll
                for (int j = 0; j < M; ++j) nd[j] = ldg(dout.p[j] + o);
                if (DUP3) nd3 = ldg(dout3b + o);
                if (n + 1 < hi) {
                    nx = ldg(xn + o);
                    if (dres) nr = ldg(dres + o);
                    nmu = mean[n + 1]; nrs = rstd[n + 1];
                }
            }
            if (n > lo) {                                        // the previous row is complete: its LayerNorm backward
                V8 t, xh;
                const V8 xv = unpack8(xprev);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    t.f[e] = aprev.f[e] + (cont ? bvv.f[e] : 0.f);
                    xh.f[e] = act ? (xv.f[e] - muprev) * rsprev : 0.f;
                }
                ln_row_bwd(red, slot, wave, lane, nw, act, inv_c, unpack8(wp), unpack8(pack8(t)), xh, rsprev, resprev, gw, gb, dx + (n - 1) * C + cc);
                slot ^= 1;
            }
            if (inside) {
#pragma unroll
                for (int e = 0; e < 8; ++e) aprev.f[e] = dsum.f[e] - bvv.f[e];
                if (CARRY && dy_last && tpos == T - 1) {         // the row ends its sample: what the next segment's first row sends it takes the
                    const V8 dl = ld8(dy_last + samp * C + cc);         // place of a continuing row's Bv -- A + Bv, formed here, + 0 where that row would add
#pragma unroll
                    for (int e = 0; e < 8; ++e) aprev.f[e] += dl.f[e];
                }
                xprev = cx; resprev = cr; muprev = mu_; rsprev = rs;
            }
            if (++tpos == T) { tpos = 0; if (CARRY) ++samp; }
        }
        if (last == hi - 1) {                                    // no successor row: the gradient of the last row is A
            V8 xh;
            const V8 xv = unpack8(xprev);
#pragma unroll
            for (int e = 0; e < 8; ++e) xh.f[e] = act ? (xv.f[e] - muprev) * rsprev : 0.f;
            ln_row_bwd(red, slot, wave, lane, nw, act, inv_c, unpack8(wp), unpack8(pack8(aprev)), xh, rsprev, resprev, gw, gb, dx + (hi - 1) * C + cc);
        }
    }
    if (act) {
        float* dst = part_ln + (size_t)blockIdx.x * 2 * C + c0;
        *reinterpret_cast<float4*>(dst) = make_float4(gw.f[0], gw.f[1], gw.f[2], gw.f[3]);
        *reinterpret_cast<float4*>(dst + 4) = make_float4(gw.f[4], gw.f[5], gw.f[6], gw.f[7]);
        *reinterpret_cast<float4*>(dst + C) = make_float4(gb.f[0], gb.f[1], gb.f[2], gb.f[3]);
        *reinterpret_cast<float4*>(dst + C + 4) = make_float4(gb.f[4], gb.f[5], gb.f[6], gb.f[7]);
#pragma unroll
        for (int j = 0; j < M; ++j) {
            float* dm = part_mu + ((size_t)blockIdx.x * M + j) * C + c0;
            *reinterpret_cast<float4*>(dm) = make_float4(gm[j].f[0], gm[j].f[1], gm[j].f[2], gm[j].f[3]);
            *reinterpret_cast<float4*>(dm + 4) = make_float4(gm[j].f[4], gm[j].f[5], gm[j].f[6], gm[j].f[7]);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// The visual token compressor's tail (VisualRWKV-v7/v7.04/src/model.py:372-373 ln_out + unpad, :524-529 AdaptiveAvgPool1d over tokens, :544-552 the
// masked scatter): (B, T, C) rows, the first `pad` of every sample are pad rows, Lin = T - pad; output i of a sample is the mean of the NORMALISED rows
// pad + [floor(i Lin / Lout), ceil((i+1) Lin / Lout)) -- the affine part of the LayerNorm commutes with the mean, so it is applied once per output:
//   out[orow[b Lout + i]] = bf16(fma(sum_t xhat[t] / len_i, w, b)),  xhat = (xn - mean) rstd,  xn = bf16(x + delta)
// With Lout <= Lin neighbouring windows share at most one row.  A workgroup walks a contiguous range of outputs in order: the shared row is the last
// row it normalised and stays in registers; only the first window of a range may normalise a row that the workgroup before it also does.  xn, mean
// and rstd of a row are written by the FIRST window that holds it (one writer per address).  The pad rows are never read.
__global__ __launch_bounds__(1024) void ln_pool_fwd_kernel(int B, int T, int pad, int Lout, int C, float eps, const uint16_t* __restrict__ x,
                                                           const uint16_t* __restrict__ delta, const uint16_t* __restrict__ w,
                                                           const uint16_t* __restrict__ b, uint16_t* __restrict__ xn, uint16_t* __restrict__ out,
                                                           float* __restrict__ mean, float* __restrict__ rstd, const long* __restrict__ orow) {
    __shared__ float red[4][MAXW][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int c0 = threadIdx.x * 8;
    const bool act = c0 < C;
    const long nout = (long)B * Lout;
    const long olo = nout * blockIdx.x / gridDim.x, ohi = nout * (blockIdx.x + 1) / gridDim.x;
    if (olo >= ohi) return;
    const int Lin = T - pad;
    const uint4 z4 = make_uint4(0, 0, 0, 0);
    const V8 wv = unpack8(act ? ldg(w + c0) : z4), bv = unpack8(act ? ldg(b + c0) : z4);
    const float inv_c = 1.f / (float)C;
    long have = -1, done = -1;                                   // the row whose loads are in flight; the row whose xhat is in `last`
    uint4 nx = z4, nd = z4;
    V8 last;
#pragma unroll
    for (int e = 0; e < 8; ++e) last.f[e] = 0.f;
    int par = 0;
    int bi = (int)(olo / Lout), i = (int)(olo - (long)bi * Lout);
    for (long o = olo; o < ohi; ++o) {
        const int s = (int)((long)i * Lin / Lout), e1 = (int)(((long)(i + 1) * Lin + Lout - 1) / Lout);
        const int own0 = (int)(((long)i * Lin + Lout - 1) / Lout);               // where window i-1 ends: rows below it are that window's
        const long base = (long)bi * T + pad;
        V8 acc;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc.f[e] = 0.f;
        for (int t = s; t < e1; ++t) {
            const long n = base + t;
            if (n != done) {
                uint4 cx, cd = z4;
                if (have == n) { cx = nx; cd = nd; }
                else {
                    cx = act ? ldg(x + n * C + c0) : z4;
                    if (act && delta) cd = ldg(delta + n * C + c0);
                }
                // the next row this workgroup normalises: t + 1 of this window, or of the next window of the same sample (t + 1 < Lin then)
                if (t + 1 < e1 || (i + 1 < Lout && o + 1 < ohi)) {
                    have = n + 1;
                    if (act) {
                        nx = ldg(x + (n + 1) * C + c0);
                        if (delta) nd = ldg(delta + (n + 1) * C + c0);
                    }
                }
                const bool own = t >= own0;
                V8 v = unpack8(cx);
                if (delta) {
                    const V8 d = unpack8(cd);
#pragma unroll
                    for (int e = 0; e < 8; ++e) v.f[e] += d.f[e];
                    const uint4 r = pack8(v);
                    if (act && own) stg(xn + n * C + c0, r);
                    v = unpack8(r);
                }
                float sm[1] = {0.f};
#pragma unroll
                for (int e = 0; e < 8; ++e) sm[0] += v.f[e];
                block_sum<1>(red, par, wave, lane, nw, sm);
                const float mu = sm[0] * inv_c;
                float q[1] = {0.f};
#pragma unroll
                for (int e = 0; e < 8; ++e) { const float d = act ? v.f[e] - mu : 0.f; q[0] = fmaf(d, d, q[0]); }
                block_sum<1>(red, par + 1, wave, lane, nw, q);
                par ^= 2;
                const float rs = rsqrtf(q[0] * inv_c + eps);
#pragma unroll
                for (int e = 0; e < 8; ++e) last.f[e] = (v.f[e] - mu) * rs;
                if (own && threadIdx.x == 0) { mean[n] = mu; rstd[n] = rs; }
                done = n;
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) acc.f[e] = t == s ? last.f[e] : acc.f[e] + last.f[e];
        }
        const float inv_len = 1.f / (float)(e1 - s);
        V8 r;
#pragma unroll
        for (int e = 0; e < 8; ++e) r.f[e] = fmaf(acc.f[e] * inv_len, wv.f[e], bv.f[e]);
        const long dst = orow ? orow[o] : o;                     // a negative row is dropped
        if (act && dst >= 0) stg(out + dst * C + c0, pack8(r));
        if (++i == Lout) { i = 0; ++bi; }
    }
}

// ... and its backward: row t of a sample collects g = sum_i dout[orow[b Lout + i]] / len_i over the one or two windows that hold it (fp32, a dropped
// output gives 0), then add_ln_bwd_kernel's row with g for dy.  The pad rows get zeros and read nothing (their mean / rstd are unwritten).  A
// workgroup walks a contiguous range of the B T rows; the next row's loads are issued before this row's reduction.
__global__ __launch_bounds__(1024) void ln_pool_bwd_kernel(int B, int T, int pad, int Lout, int C, const uint16_t* __restrict__ dout,
                                                           const long* __restrict__ orow, const uint16_t* __restrict__ xn,
                                                           const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           const uint16_t* __restrict__ w, uint16_t* __restrict__ dx, float* __restrict__ part) {
    __shared__ float red[2][MAXW][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int c0 = threadIdx.x * 8;
    const bool act = c0 < C;
    const long ntok = (long)B * T;
    const long lo = ntok * blockIdx.x / gridDim.x, hi = ntok * (blockIdx.x + 1) / gridDim.x;
    const int Lin = T - pad;
    const uint4 z4 = make_uint4(0, 0, 0, 0);
    const V8 wv = unpack8(act ? ldg(w + c0) : z4);
    const float inv_c = 1.f / (float)C;
    V8 gw, gb;
#pragma unroll
    for (int e = 0; e < 8; ++e) { gw.f[e] = 0.f; gb.f[e] = 0.f; }
    struct Row { uint4 x, d0, d1; float s0, s1, mu, rs; };
    // everything row (bb, t >= pad) needs: its xn and statistics, the gradient rows of its windows and their 1 / len
    auto fetch = [&](long n, int bb, int t) {
        Row r{z4, z4, z4, 0.f, 0.f, 0.f, 0.f};
        const int tt = t - pad;
        const int i0 = (int)((long)tt * Lout / Lin), i1 = (int)(((long)(tt + 1) * Lout + Lin - 1) / Lin) - 1;
        auto len = [&](int i) { return (int)(((long)(i + 1) * Lin + Lout - 1) / Lout) - (int)((long)i * Lin / Lout); };
        const long o0 = (long)bb * Lout + i0;
        const long r0 = orow ? orow[o0] : o0;
        if (act && r0 >= 0) r.d0 = ldg(dout + r0 * C + c0);
        r.s0 = 1.f / (float)len(i0);
        if (i1 > i0) {
            const long r1 = orow ? orow[o0 + 1] : o0 + 1;
            if (act && r1 >= 0) r.d1 = ldg(dout + r1 * C + c0);
            r.s1 = 1.f / (float)len(i0 + 1);
        }
        if (act) r.x = ldg(xn + n * C + c0);
        r.mu = mean[n]; r.rs = rstd[n];
        return r;
    };
    int bi = (int)(lo / T), t = (int)(lo - (long)bi * T);
    Row nxt{z4, z4, z4, 0.f, 0.f, 0.f, 0.f};
    if (lo < hi && t >= pad) nxt = fetch(lo, bi, t);
    int slot = 0;
    for (long n = lo; n < hi; ++n) {
        const Row cur = nxt;
        const bool real = t >= pad;
        if (++t == T) { t = 0; ++bi; }
        if (n + 1 < hi && t >= pad) nxt = fetch(n + 1, bi, t);
        if (!real) {                                             // workgroup-uniform
            if (act) stg(dx + n * C + c0, z4);
            continue;
        }
        const V8 a0 = unpack8(cur.d0), a1 = unpack8(cur.d1), xv = unpack8(cur.x);
        V8 xh, g;
        float s[2] = {0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float d = fmaf(a1.f[e], cur.s1, a0.f[e] * cur.s0);
            xh.f[e] = act ? (xv.f[e] - cur.mu) * cur.rs : 0.f;
            g.f[e] = d * wv.f[e];
            s[0] += g.f[e];
            s[1] = fmaf(g.f[e], xh.f[e], s[1]);
            gw.f[e] = fmaf(d, xh.f[e], gw.f[e]);
            gb.f[e] += d;
        }
        block_sum<2>(red, slot, wave, lane, nw, s);
        slot ^= 1;
        const float c1 = s[0] * inv_c, c2 = s[1] * inv_c;
        V8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o.f[e] = fmaf(cur.rs, g.f[e] - c1 - xh.f[e] * c2, 0.f);
        if (act) stg(dx + n * C + c0, pack8(o));
    }
    if (act) {
        float* dst = part + (size_t)blockIdx.x * 2 * C + c0;
        *reinterpret_cast<float4*>(dst) = make_float4(gw.f[0], gw.f[1], gw.f[2], gw.f[3]);
        *reinterpret_cast<float4*>(dst + 4) = make_float4(gw.f[4], gw.f[5], gw.f[6], gw.f[7]);
        *reinterpret_cast<float4*>(dst + C) = make_float4(gb.f[0], gb.f[1], gb.f[2], gb.f[3]);
        *reinterpret_cast<float4*>(dst + C + 4) = make_float4(gb.f[4], gb.f[5], gb.f[6], gb.f[7]);
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// The RWKV vision encoder's tail (VisualRWKV-v7/v7.10/src/model.py:392-394 ln_out and the ImageNet head's mean over tokens, :510-526 the masked
// scatter): (B, L, C) rows, every row is normalised once and leaves twice --
//   out[orow[b L + t]] = bf16(fma(xhat, w, b))  (add_ln_fwd_kernel's row, bit for bit),   pooled[b] = bf16(fma(sum_t xhat[b, t] / L, w, b))
// with xhat = (xn - mean) rstd, xn = bf16(x + delta): the affine part commutes with the mean (ln_pool_fwd_kernel's convention).  A dropped row
// (orow < 0) still counts in the mean.  Workgroup (b, p) of B P walks rows [L p / P, L (p + 1) / P) of sample b with the next row in flight and
// leaves one fp32 partial row of the sum; ln_mean_finish_kernel adds the P partial rows of a sample in order: deterministic, no atomics.
__global__ __launch_bounds__(1024) void ln_scatter_mean_fwd_kernel(int L, int P, int C, float eps, const uint16_t* __restrict__ x,
                                                                   const uint16_t* __restrict__ delta, const uint16_t* __restrict__ w,
                                                                   const uint16_t* __restrict__ b, uint16_t* __restrict__ xn, uint16_t* __restrict__ out,
                                                                   float* __restrict__ mean, float* __restrict__ rstd, const long* __restrict__ orow,
                                                                   float* __restrict__ part) {
    __shared__ float red[4][MAXW][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int c0 = threadIdx.x * 8;
    const bool act = c0 < C;
    const long bi = blockIdx.x / P;
    const int pi = (int)(blockIdx.x - bi * P);
    const long lo = bi * L + (long)L * pi / P, hi = bi * L + (long)L * (pi + 1) / P;
    const uint4 z4 = make_uint4(0, 0, 0, 0);
    const V8 wv = unpack8(act ? ldg(w + c0) : z4), bv = unpack8(act ? ldg(b + c0) : z4);
    const float inv_c = 1.f / (float)C;
    V8 acc;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc.f[e] = 0.f;
    uint4 nx = z4, nd = z4;
    if (lo < hi && act) { nx = ldg(x + lo * C + c0); if (delta) nd = ldg(delta + lo * C + c0); }
    for (long n = lo; n < hi; ++n) {
        const uint4 cx = nx, cd = nd;
        if (n + 1 < hi && act) {
            nx = ldg(x + (n + 1) * C + c0);
            if (delta) nd = ldg(delta + (n + 1) * C + c0);
        }
        V8 v = unpack8(cx);
        if (delta) {
            const V8 d = unpack8(cd);
#pragma unroll
            for (int e = 0; e < 8; ++e) v.f[e] += d.f[e];
            const uint4 r = pack8(v);
            if (act) stg(xn + n * C + c0, r);
            v = unpack8(r);
        }
        const int par = (int)(n & 1) * 2;
        float s[1] = {0.f};
#pragma unroll
        for (int e = 0; e < 8; ++e) s[0] += v.f[e];
        block_sum<1>(red, par, wave, lane, nw, s);
        const float mu = s[0] * inv_c;
        float q[1] = {0.f};
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float t = act ? v.f[e] - mu : 0.f; q[0] = fmaf(t, t, q[0]); }
        block_sum<1>(red, par + 1, wave, lane, nw, q);
        const float rs = rsqrtf(q[0] * inv_c + eps);
        V8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float xh = (v.f[e] - mu) * rs;
            acc.f[e] += xh;
            o.f[e] = fmaf(xh, wv.f[e], bv.f[e]);
        }
        const long orow_n = orow ? orow[n] : n;                 // a negative row is dropped
        if (act && orow_n >= 0) stg(out + orow_n * C + c0, pack8(o));
        if (threadIdx.x == 0) { mean[n] = mu; rstd[n] = rs; }
    }
    if (act) {
        float* dst = part + (size_t)blockIdx.x * C + c0;
        *reinterpret_cast<float4*>(dst) = make_float4(acc.f[0], acc.f[1], acc.f[2], acc.f[3]);
        *reinterpret_cast<float4*>(dst + 4) = make_float4(acc.f[4], acc.f[5], acc.f[6], acc.f[7]);
    }
}

// pooled[b, c] = bf16(fma(sum_p part[b, p, c] / L, w[c], b[c])); one thread per element
__global__ __launch_bounds__(256) void ln_mean_finish_kernel(long n, int P, int C, float inv_l, const float* __restrict__ part, const uint16_t* __restrict__ w,
                                                             const uint16_t* __restrict__ b, uint16_t* __restrict__ pooled) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long bi = i / C;
    const int c = (int)(i - bi * C);
    const float* src = part + (size_t)bi * P * C + c;
    float t = src[0];
    for (int p = 1; p < P; ++p) t += src[(size_t)p * C];
    pooled[i] = (uint16_t)f32_to_bf16_bits(fmaf(t * inv_l, bf16_to_f32(w[c]), bf16_to_f32(b[c])));
}

// ... and its backward: row (b, t) collects g = dout[orow[b L + t]] (0 for a dropped row, or without dout) + dpooled[b] / L (fp32; without dpooled g is
// dout's row itself), then add_ln_bwd_kernel's row with g for dy and no residual gradient.  Same ranges, partial rows and prefetch as that kernel.
__global__ __launch_bounds__(1024) void ln_gather_mean_bwd_kernel(long ntok, int L, int C, const uint16_t* __restrict__ dout, const long* __restrict__ orow,
                                                                  const uint16_t* __restrict__ dpooled, const uint16_t* __restrict__ xn,
                                                                  const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                  const uint16_t* __restrict__ w, uint16_t* __restrict__ dx, float* __restrict__ part) {
    __shared__ float red[2][MAXW][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int c0 = threadIdx.x * 8;
    const bool act = c0 < C;
    const long lo = ntok * blockIdx.x / gridDim.x, hi = ntok * (blockIdx.x + 1) / gridDim.x;
    const uint4 z4 = make_uint4(0, 0, 0, 0);
    const V8 wv = unpack8(act ? ldg(w + c0) : z4);
    const float inv_c = 1.f / (float)C, inv_l = 1.f / (float)L;
    V8 gw, gb;
#pragma unroll
    for (int e = 0; e < 8; ++e) { gw.f[e] = 0.f; gb.f[e] = 0.f; }
    struct Row { uint4 y, p, x; float mu, rs; };
    auto fetch = [&](long n) {
        Row r{z4, z4, z4, 0.f, 0.f};
        if (act) {
            if (dout) { const long o = orow ? orow[n] : n; if (o >= 0) r.y = ldg(dout + o * C + c0); }
            if (dpooled) r.p = *reinterpret_cast<const uint4*>(dpooled + (n / L) * C + c0);      // L rows share it: cached
            r.x = ldg(xn + n * C + c0);
        }
        r.mu = mean[n]; r.rs = rstd[n];
        return r;
    };
    Row nxt{z4, z4, z4, 0.f, 0.f};
    if (lo < hi) nxt = fetch(lo);
    for (long n = lo; n < hi; ++n) {
        const Row cur = nxt;
        if (n + 1 < hi) nxt = fetch(n + 1);
        V8 d = unpack8(cur.y);
        if (dpooled) {
            const V8 dp = unpack8(cur.p);
#pragma unroll
            for (int e = 0; e < 8; ++e) d.f[e] = fmaf(dp.f[e], inv_l, d.f[e]);
        }
        const V8 xv = unpack8(cur.x);
        V8 xh, g;
        float s[2] = {0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            xh.f[e] = act ? (xv.f[e] - cur.mu) * cur.rs : 0.f;
            g.f[e] = d.f[e] * wv.f[e];
            s[0] += g.f[e];
            s[1] = fmaf(g.f[e], xh.f[e], s[1]);
            gw.f[e] = fmaf(d.f[e], xh.f[e], gw.f[e]);
            gb.f[e] += d.f[e];
        }
        block_sum<2>(red, (int)(n & 1), wave, lane, nw, s);
        const float c1 = s[0] * inv_c, c2 = s[1] * inv_c;
        V8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o.f[e] = fmaf(cur.rs, g.f[e] - c1 - xh.f[e] * c2, 0.f);
        if (act) stg(dx + n * C + c0, pack8(o));
    }
    if (act) {
        float* dst = part + (size_t)blockIdx.x * 2 * C + c0;
        *reinterpret_cast<float4*>(dst) = make_float4(gw.f[0], gw.f[1], gw.f[2], gw.f[3]);
        *reinterpret_cast<float4*>(dst + 4) = make_float4(gw.f[4], gw.f[5], gw.f[6], gw.f[7]);
        *reinterpret_cast<float4*>(dst + C) = make_float4(gb.f[0], gb.f[1], gb.f[2], gb.f[3]);
        *reinterpret_cast<float4*>(dst + C + 4) = make_float4(gb.f[4], gb.f[5], gb.f[6], gb.f[7]);
    }
}

// dst[i] = src[idx[i]] on rows of C bf16 (cv = C / 8 16-byte pieces per row; idx int32, or int64 with IDX64): the routed channel mix's way back to
// token order, and with the inverse index that step's backward
template <bool IDX64>
__global__ __launch_bounds__(256) void row_gather_kernel(long nvec, int cv, const uint16_t* __restrict__ src, const void* __restrict__ idx,
                                                         uint16_t* __restrict__ dst) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (long)gridDim.x * blockDim.x) {
        const long r = i / cv, c = i - r * cv;
        const long sr = IDX64 ? reinterpret_cast<const long*>(idx)[r] : (long)reinterpret_cast<const int*>(idx)[r];
        stg(dst + i * 8, ldg(src + (sr * cv + c) * 8));
    }
}

}  // namespace vln
