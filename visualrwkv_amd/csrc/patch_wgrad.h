// Weight gradient of a trained patch embedding, Conv2d(3, N, 16, 16) with stride 16 (VisualRWKV-v7/v7.10/src/model.py:371,378: vrwkv.emb):
//   dW[n, (c 16 + py) 16 + px] = sum_{b,m} dout[b Mimg + m, n] pixels[b, c, 16 gy + py, 16 gx + px],   m = gy gw + gx
// This is wgrad_big.h's product C = A^T B with A = dout (M x N) and B = the unfolded images (M x 768) -- which are never stored: K = 768 is three
// tile columns, one per colour channel, and a token's 256 columns of one channel are 16 pixel-row segments of 32 bytes = the 32 16-byte slots of
// its 512-byte LDS row, so only the SOURCE address of the B tile's LDS-DMA differs from wgrad_big_kernel (same 256 x 256 tile, 32-row stages,
// three-stage ring, XOR swizzle on the source slot, transposing reads, split over M, wgrad_big_reduce).  The body below is that kernel's with
// the B requests replaced; templating the original on the source changed its register allocation, so it is a sibling and not an instantiation.
// Token -> (image, patch row, patch column) takes two divisions per lane and request: by multiplication (Div below), the divisors are uniform.
// Pixel byte offsets are 32-bit: the launcher refuses image batches of 4 GiB and more.
#pragma once
#include <wgrad_big.h>

namespace wgp {

using namespace wgb;

// n / d for 0 <= n < 2^31 by one multiplication (Granlund & Montgomery, N = 31): with l = ceil(log2 d) >= 1 and mul = floor(2^(31+l) / d) + 1 < 2^32,
// 2^(31+l) < mul d <= 2^(31+l) + 2^l, so floor(n mul / 2^(31+l)) = floor(n / d).  d == 1: mul == 0 marks the identity.
struct Div {
    unsigned mul, shift;
    static Div make(unsigned d) {
        if (d <= 1) return Div{0u, 0u};
        unsigned l = 1;
        while ((1ull << l) < d) ++l;
        return Div{(unsigned)((1ull << (31 + l)) / d + 1ull), l - 1};
    }
    __host__ __device__ inline unsigned div(unsigned n) const { return mul ? (unsigned)(((unsigned long long)n * mul) >> 32) >> shift : n; }
};

struct Args {
    long M;
    int N1, N2, S;                  // N2 = 768
    const uint16_t* A;              // dout (M, N1)
    const uint16_t* B;              // pixels (B, 3, Himg, Wimg)
    float* part;                    // [S][N1][768] fp32 (S > 1)
    uint16_t* out;                  // (N1, 768) bf16 (S == 1)
    int Mimg, gw, Himg, Wimg;       // tokens per image, patches per image row, image size in pixels
    Div dimg, dgw;                  // / Mimg, / gw
};

__global__ __launch_bounds__(512) void wgrad_patch_kernel(Args p) {
    char* lds = dyn_lds();                             // [STAGES][A tile | B tile]
    const int tid = threadIdx.x, lane = tid & 63, wave = uniform_i32(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    // block id -> (slice, tile column, tile row) with the tile row in the low bits: ids that are equal mod 8 share A's column block
    const int T1 = p.N1 / TM, T2 = p.N2 / TN;
    const int i1 = blockIdx.x % T1, rest = blockIdx.x / T1, i2 = rest % T2, sl = rest / T2;
    const long nst = p.M / KT;
    const long s0 = nst * sl / p.S, s1 = nst * (sl + 1) / p.S;
    // ---- requests: a stage is 16 + 16 instructions of 1 KB (2 rows of 512 B each); wave w issues instructions 2w, 2w+1 of A and of B.
    // lane l of instruction j: row 2j + (l >> 5), LDS slot l & 31 <- source slot (l & 31) ^ 4 (row & 3)
    // B: LDS slot l & 31 of token row `row` <- source slot s = (l & 31) ^ 4 (row & 3) = pixels[b, c, 16 gy + s / 2, 16 gx + 8 (s & 1) ..], c = i2.
    // rowB[q]: the lane's row of the stage; fixB[q]: the byte offset of (channel c, pixel row s / 2, half s & 1) inside image 0, patch (0, 0)
    unsigned offA[2], rowB[2], fixB[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const unsigned row = 2u * (2u * wave + q) + ((unsigned)lane >> 5), slot = ((unsigned)lane & 31u) ^ (4u * (row & 3u));
        offA[q] = row * (unsigned)p.N1 * 2u + 16u * slot;
        rowB[q] = row;
        fixB[q] = (((unsigned)i2 * (unsigned)p.Himg + (slot >> 1)) * (unsigned)p.Wimg + 8u * (slot & 1u)) * 2u;
    }
    const char* gA = reinterpret_cast<const char*>(p.A + (size_t)s0 * KT * p.N1 + (size_t)i1 * TM);
    const char* gB = reinterpret_cast<const char*>(p.B);
    const size_t stepA = (size_t)KT * p.N1 * 2;
    const unsigned img_bytes = 3u * (unsigned)p.Himg * (unsigned)p.Wimg * 2u, prow_bytes = 16u * (unsigned)p.Wimg * 2u;
    const unsigned lds0 = lds_addr_u32(lds);
    unsigned tok = (unsigned)s0 * KT;                   // the first token row of the next stage to request
    auto request = [&](int slot) {                      // the next stage (gA / tok advance) into LDS stage `slot` (compile-time after unrolling)
        const unsigned d = lds0 + (unsigned)slot * (2u * OPB) + (unsigned)(2 * wave) * 1024u;
        unsigned offB[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {                   // b is per lane: a stage may straddle images
            const unsigned t = tok + rowB[q], b = p.dimg.div(t), m = t - b * (unsigned)p.Mimg, gy = p.dgw.div(m), gx = m - gy * (unsigned)p.gw;
            offB[q] = b * img_bytes + gy * prow_bytes + gx * 32u + fixB[q];
        }
        lds_dma16_lean<0>(gA, offA[0], d);
        lds_dma16_lean<0>(gA, offA[1], d + 1024u);
        lds_dma16_lean<0>(gB, offB[0], d + OPB);
        lds_dma16_lean<0>(gB, offB[1], d + OPB + 1024u);
        gA += stepA; tok += KT;
    };
    // ---- operand fetch: ds_read_b64_tr_b16 on a [32][256] image.  v_mfma_f32_32x32x16_bf16: lane l holds row / column (l & 31), k = 8 (l >> 5) + e.
    // 16-lane group (l >> 4): column block 16 ((l >> 4) & 1) of the 32, rows 8 (l >> 5) + 4h + ((l & 15) >> 2), h = 0, 1; the lane
    // points at 4 consecutive columns 4 (l & 3) of its row.  Physical slot = (column / 8) ^ 4 (row & 3).  One byte offset per
    // fragment and lane, computed once: stage, k16 (+ 8 KB) and h (+ 2 KB) are immediates of the read.
    const int rq = (lane & 15) >> 2;                                   // row & 3 of both reads (8 (l>>5) + 4h are multiples of 4)
    const int cl = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);            // column inside a 32-column MFMA tile
    const int rbase = 8 * (lane >> 5) + rq;
    auto frag_off = [&](int col0) {
        const int col = col0 + cl;
        return rbase * ROWB + (((col >> 3) ^ (4 * rq)) * 16) + (col & 7) * 2;
    };
    int fa[4], fb[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) fa[i] = frag_off(128 * wr + 32 * i);
#pragma unroll
    for (int j = 0; j < 2; ++j) fb[j] = OPB + frag_off(64 * wc + 32 * j);
    auto frag = [&](const char* stage, int off, int k16) -> bf16x8 {
        const char* base = stage + off + k16 * 16 * ROWB;
        return mk8(lds_read_tr16(reinterpret_cast<const uint16_t*>(base)), lds_read_tr16(reinterpret_cast<const uint16_t*>(base + 4 * ROWB)));
    };
    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    auto compute = [&](int slot) {
        const char* st = lds + slot * (2 * OPB);
#pragma unroll
        for (int k16 = 0; k16 < 2; ++k16) {
            bf16x8 a[4], b[2];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = frag(st, fa[i], k16);
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = frag(st, fb[j], k16);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = mfma_32x32x16_bf16(a[i], b[j], acc[i][j]);
        }
    };
    // One stage: request stage s + STAGES - 1 into the slot stage s - 1 has left, multiply stage s, wait for this wave's requests of
    // stage s + 1 (all but the newest 4 (STAGES - 2)), barrier.  Unrolled by STAGES so that every LDS address is lane offset + immediate.
    const long ns = s1 - s0;
    long issued = 0;
    if (ns > 0) {
#pragma unroll
        for (int q = 0; q < STAGES - 1; ++q) if (q < ns) { request(q); ++issued; }
        if (issued > 1) vmem_wait<4 * (STAGES - 2)>(); else vmem_drain();
        if (ns < STAGES) vmem_drain();
        block_sync_lds();
        long s = 0;
        for (; s + STAGES <= ns - (STAGES - 1); s += STAGES) {        // steady state: every stage of the group requests another
#pragma unroll
            for (int q = 0; q < STAGES; ++q) {
                request((q + STAGES - 1) % STAGES);
                compute(q);
                vmem_wait<4 * (STAGES - 2)>();
                block_sync_lds();
            }
        }
        for (; s < ns; ++s) {                                          // the last stages: nothing left to request beyond ns
            const int q = (int)(s % STAGES);
            const bool more = s + STAGES - 1 < ns;
            if (more) request((q + STAGES - 1) % STAGES);
            compute(q);
            if (more) vmem_wait<4 * (STAGES - 2)>(); else vmem_drain();
            block_sync_lds();
        }
    }
    // ---- epilogue.  C/D of 32x32: register r <-> row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31
    const int rowl = 4 * (lane >> 5), coll = lane & 31;
    if (p.S > 1) {
        float* out = p.part + ((size_t)sl * p.N1 + (size_t)i1 * TM + 128 * wr) * p.N2 + (size_t)i2 * TN + 64 * wc;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    out[(size_t)(32 * i + (r & 3) + 8 * (r >> 2) + rowl) * p.N2 + 32 * j + coll] = acc[i][j][r];
    } else {
        uint16_t* out = p.out + ((size_t)i1 * TM + 128 * wr) * p.N2 + (size_t)i2 * TN + 64 * wc;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    out[(size_t)(32 * i + (r & 3) + 8 * (r >> 2) + rowl) * p.N2 + 32 * j + coll] = (uint16_t)f32_to_bf16_bits(acc[i][j][r]);
    }
}

// dbias[n] = sum_m dout[m, n]: workgroup (column block of 256, row slice g of G) -> one fp32 partial row; a thread sums 8 columns over one of 8
// row lanes, the row lanes are joined through LDS in a fixed order; colsum_finish_kernel adds the G partial rows in order and rounds once.
__global__ __launch_bounds__(256) void colsum_part_kernel(long M, int N, const uint16_t* __restrict__ x, float* __restrict__ part) {
    __shared__ float red[8][256];
    const int cg = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const int col = blockIdx.x * 256 + 8 * cg;
    const long lo = M * blockIdx.y / gridDim.y, hi = M * (blockIdx.y + 1) / gridDim.y;
    float a[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = 0.f;
    for (long m = lo + rl; m < hi; m += 8) {
        const uint4 u = *reinterpret_cast<const uint4*>(x + m * N + col);
        a[0] += bf16_lo(u.x); a[1] += bf16_hi(u.x); a[2] += bf16_lo(u.y); a[3] += bf16_hi(u.y);
        a[4] += bf16_lo(u.z); a[5] += bf16_hi(u.z); a[6] += bf16_lo(u.w); a[7] += bf16_hi(u.w);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) red[rl][8 * cg + e] = a[e];
    __syncthreads();
    float t = red[0][threadIdx.x];
#pragma unroll
    for (int r = 1; r < 8; ++r) t += red[r][threadIdx.x];
    part[(size_t)blockIdx.y * N + blockIdx.x * 256 + threadIdx.x] = t;
}
__global__ __launch_bounds__(256) void colsum_finish_kernel(int G, int N, const float* __restrict__ part, uint16_t* __restrict__ out) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float t = part[n];
    for (int g = 1; g < G; ++g) t += part[(size_t)g * N + n];
    out[n] = (uint16_t)f32_to_bf16_bits(t);
}

}  // namespace wgp
