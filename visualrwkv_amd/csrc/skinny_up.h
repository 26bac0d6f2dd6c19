// Write-wide product of a LoRA pair: out (M x C) = a (M x R) . w, a narrow activation (R = 32 .. 256) times a small factor -- gfx950.
//
// These are h @ w2 of the w / a / g / v-gate pairs of RWKV_Tmix_x070 and the input gradients dh @ w1^T of their down-projections
// (VisualRWKV-v7/v7.00/src/model.py:176,181-183 and autograd's mm).  There is no arithmetic to win (16-44 GFLOP per product at
// M = 41 984, C = 2048); the product writes 172 MB and reads 5-21 MB, so it is worth what its stores are worth.
//
// The product is computed transposed, out^T = w^T a^T, with v_mfma_f32_32x32x16_bf16:
//   A operand = w^T  (i = channel, k): a wave's 64 channels x R, fetched ONCE and kept in registers for the whole launch (2 R/16 fragments of
//               4 registers).  w as (C, R) (the input gradient: w1) is read as it lies, 16 bytes per lane and fragment; w as (R, C) (the forward:
//               w2) goes through LDS in 32-row pieces, stored as it lies and fetched with ds_read_b64_tr_b16 (as wgrad_big.h): no transposed copy.
//   B operand = a^T  (k, j = token): lane = token (l & 31), 8 consecutive k = 16 bytes of a's row, read as it lies; the NEXT tile's loads are
//               issued before the current tile is multiplied and stored.  R <= 96 and 160: every wave loads the tile into registers.  R = 128
//               and 256: once per workgroup into LDS by DMA, two buffers, one workgroup barrier per tile (measured at R = 256, M = 41 984,
//               C = 2048: 88.6 / 82.3 us as registers, 45.6 / 48.0 us through LDS, for w as (R, C) / (C, R)).
//   C/D              lane = token, registers = channels (r & 3) + 8 (r >> 2) + 4 (l >> 5): four packed 8-byte pieces per 32 channels.
// The packed tile goes through the wave's own LDS image ([32 tokens][64 channels], rows padded to 144 B) and leaves row-major: one store
// instruction = 8 rows x 128 contiguous bytes, 16 bytes per lane.  Only the wave itself touches its image.
// The sums are the library's: at all six ranks and both layouts the output is bit-equal to hipBLASLt's tuned kernel for the shape
// (benchmarks/lora_gemm_micro.py compares them).
//
// A workgroup = NW waves = a strip of 64 NW columns (256; 128 where C is an odd multiple of 128) x the row tiles rg, rg + G, ... of its row group rg.
// Workgroups that share a row group have ids equal mod 8 (one XCD: its L2 serves the narrow tile to all strips, as in wgrad_big.h).
// A workgroup never waits for another one (no flags, no atomics): it may run beside a library GEMM.
#pragma once
#include <gfx950_prims.h>

namespace skup {

constexpr int TR = 32;                    // tokens per tile (the MFMA's j)
constexpr int WC = 64;                    // columns per wave (two 32-channel MFMA tiles)
constexpr int ROWB = WC * 2 + 16;         // bytes of one row of a wave's LDS image; 36 dwords: rows r and r + 1 sit 36 banks apart
constexpr int WAVE_LDS = TR * ROWB;       // 4608 B per wave

// ranks whose narrow tile goes through LDS (a row of 16 or 32 slots: the XOR needs a power of two)
constexpr bool shared_tile(int R) { return R == 128 || R == 256; }
constexpr int lds_bytes(int R, int NW) { return (shared_tile(R) ? 2 * TR * R * 2 : 0) + NW * WAVE_LDS; }

struct Args {
    long M;
    int C, G;                             // G: row groups, a multiple of 8
    const uint16_t* a;                    // (M, R)
    const uint16_t* w;                    // (R, C), or (C, R) for CXR
    uint16_t* out;                        // (M, C)
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
DEVFN bf16x8 frag8(u32x4 v) { return __builtin_bit_cast(bf16x8, v); }
DEVFN bf16x8 frag8(uint2 lo, uint2 hi) {
    u32x4 v = {lo.x, lo.y, hi.x, hi.y};
    return __builtin_bit_cast(bf16x8, v);
}

template <int R, int NW, bool CXR>
__global__ __launch_bounds__(64 * NW) void skinny_up_kernel(Args p) {
    constexpr int KS = R / 16;                                         // k steps of the MFMA
    constexpr bool SHARED = shared_tile(R);
    constexpr int TILEB = TR * R * 2, SLOTS = R / 8;                   // bytes of a narrow tile, 16-byte slots of one of its rows
    const int lane = threadIdx.x & 63, wave = uniform_i32(threadIdx.x >> 6);
    // block id -> (row group, strip): the low three bits of the id belong to the row group, so its strips sit on one XCD
    const int NS = p.C / (WC * NW), id = blockIdx.x;
    const int strip = (id >> 3) % NS;
    const long rg = (long)(id / (8 * NS)) * 8 + (id & 7);
    const long ntile = (p.M + TR - 1) / TR;
    if (rg >= ntile) return;                                           // the whole workgroup: G is rounded up to 8
    const int c0 = (strip * NW + wave) * WC;
    char* img = dyn_lds() + (SHARED ? 2 * TILEB : 0) + wave * WAVE_LDS;
    const int tok = lane & 31, kh = lane >> 5;
    const int srow = lane >> 3, sch = lane & 7;                        // row-major side of the image: row srow + 8 i, 16-byte piece sch

    // ---- the wave's 64 columns of w as A fragments: wf[j][ks] = w^T[c0 + 32 j + tok][16 ks + 8 kh + e]
    bf16x8 wf[2][KS];
    if (CXR) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
                wf[j][ks] = frag8(*reinterpret_cast<const u32x4*>(p.w + (size_t)(c0 + 32 * j + tok) * R + 16 * ks + 8 * kh));
    } else {
        // 32 rows of w (k) x the wave's 64 columns into the image as they lie, then transposing reads: 16-lane group (l >> 4): column block
        // 16 ((l >> 4) & 1) of the 32, rows 8 kh + 4 h + ((l & 15) >> 2), h = 0, 1; the lane points at the 4 columns 4 (l & 3) of its row
        const char* tr = img + (8 * kh + ((lane & 15) >> 2)) * ROWB + (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;
#pragma unroll
        for (int ch = 0; ch < R / 32; ++ch) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = srow + 8 * i;
                *reinterpret_cast<u32x4*>(img + row * ROWB + 16 * sch) =
                    *reinterpret_cast<const u32x4*>(p.w + (size_t)(32 * ch + row) * p.C + c0 + 8 * sch);
            }
            wave_lds_fence();
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const char* b = tr + 16 * kk * ROWB + 64 * j;
                    wf[j][2 * ch + kk] = frag8(lds_read_tr16(reinterpret_cast<const uint16_t*>(b)),
                                               lds_read_tr16(reinterpret_cast<const uint16_t*>(b + 4 * ROWB)));
                }
            wave_lds_fence();
        }
    }

    // the tile's accumulators out: registers 4 q .. 4 q + 3 of tile j = channels 32 j + 8 q + 4 kh .. + 3 of token `tok`: one rounding, 8 bytes into
    // the token's row of the image; then the image row-major.  Rows past M (the last tile) are not stored.
    auto store_tile = [&](long t, const f32x16 (&acc)[2]) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                *reinterpret_cast<uint2*>(img + tok * ROWB + (32 * j + 8 * q + 4 * kh) * 2) =
                    make_uint2(cvt_pk_bf16(acc[j][4 * q], acc[j][4 * q + 1]), cvt_pk_bf16(acc[j][4 * q + 2], acc[j][4 * q + 3]));
        wave_lds_fence();
        // the output is written once and read by the next kernel after 172 MB of other rows: non-temporal, as the row kernels of tmix_fused.hip
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = srow + 8 * i;
            const u32x4 v = *reinterpret_cast<const u32x4*>(img + row * ROWB + 16 * sch);
            const long grow = t * TR + row;
            if (grow < p.M) __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(p.out + grow * p.C + c0 + 8 * sch));
        }
        wave_lds_fence();
    };

    // ---- row loop.  Rows past M read row M - 1 again.
    if constexpr (SHARED) {
        // Wide ranks: the tile (32 rows x 2 R bytes, contiguous in memory) comes in ONCE per workgroup by LDS-DMA, 1 KB per instruction, into one of two
        // buffers, and every wave reads its B fragments from there.  (As registers of every wave, a lane's 16 bytes sit a whole row apart from its
        // neighbour's: R / 16 requests of 32 lines each per wave and tile, four times over, and two tiles of them leave one wave per SIMD.)  A row is
        // one or two bank periods, so its 16-byte slots are XOR-ed with the row number -- on the DMA's SOURCE address, as in wgrad_big.h: the 16 lanes
        // = 16 rows of one read phase then hit 16 different slots.
        constexpr int NI = R / 16 / NW;                                // DMA instructions per wave and tile
        char* tile = dyn_lds();
        int drow[NI];
        unsigned dsrc[NI];
#pragma unroll
        for (int q = 0; q < NI; ++q) {
            const int b = 1024 * (wave * NI + q) + 16 * lane, r = b / (2 * R), s = (b % (2 * R)) / 16;
            drow[q] = r;
            dsrc[q] = 16u * (unsigned)(s ^ (r & (SLOTS - 1)));
        }
        auto request = [&](long t, int buf) {
#pragma unroll
            for (int q = 0; q < NI; ++q) {
                long row = t * TR + drow[q];
                if (row >= p.M) row = p.M - 1;
                lds_dma16(reinterpret_cast<const char*>(p.a) + row * (2L * R) + dsrc[q], tile + buf * TILEB + 1024 * (wave * NI + q));
            }
        };
        const char* brow = tile + tok * (2 * R);
        const int bx = tok & (SLOTS - 1);
        request(rg, 0);
        vmem_drain();
        int buf = 0;
        for (long t = rg; t < ntile; t += p.G) {
            // every wave's part of tile t has landed (waited for below), and every wave is done reading the other buffer
            block_sync_lds();
            const bool more = t + p.G < ntile;
            if (more) request(t + p.G, buf ^ 1);
            f32x16 acc[2];
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const bf16x8 b = frag8(*reinterpret_cast<const u32x4*>(brow + buf * TILEB + 16 * ((2 * ks + kh) ^ bx)));
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[j] = mfma_32x32x16_bf16(wf[j][ks], b, acc[j]);
            }
            store_tile(t, acc);
            // the requests went out before this tile's four stores (a tile with a successor is a full one: all four are issued): all but those four
            if (more) vmem_wait<4>();
            buf ^= 1;
        }
    } else {
        auto load_a = [&](long t, u32x4 (&dst)[KS]) {
            long row = t * TR + tok;
            if (row >= p.M) row = p.M - 1;
            const uint16_t* src = p.a + row * R + 8 * kh;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) dst[ks] = *reinterpret_cast<const u32x4*>(src + 16 * ks);
        };
        u32x4 cur[KS], nxt[KS];
        load_a(rg, cur);
        for (long t = rg; t < ntile; t += p.G) {
            const bool more = t + p.G < ntile;
            if (more) load_a(t + p.G, nxt);
            f32x16 acc[2];
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[j] = mfma_32x32x16_bf16(wf[j][ks], frag8(cur[ks]), acc[j]);
            store_tile(t, acc);
            if (more) {
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) cur[ks] = nxt[ks];
            }
        }
    }
}

}  // namespace skup
