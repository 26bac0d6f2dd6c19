// Sampling head of the decode step: one logits row -> the picked token, its logit and probability, and the token's embedding row as the
// next step's input.  The pick follows PIPELINE.sample_logits of the `rwkv` package, which the reference's applications call on the output
// of VisualRWKV.generate's model pass (VisualRWKV-v7/v7.00/src/model.py:496-530): the top-p cut on the temperature-1 softmax, the
// temperature on what is left -- made deterministic (inverse CDF on a caller-supplied u, ties at the cut-off kept):
//   1. p = softmax(l)                                      2. K = { i : p_i >= c }, c = the first descending value whose running sum reaches top_p
//   3. q_i = exp((l_i - max l) / temperature), i in K      4. token = first i in K (index order) with sum_{j <= i, j in K} q_j > u sum_K q
//   5. l_token, p_token = exp(l_token - max l) / sum exp(l - max l)
// One workgroup of 1024 threads per row; the row (at most 65 536 bf16 = 128 KB) is read from memory once and parked in LDS as keys, in
// 16-byte pieces laid out [piece of the thread][thread] (a thread only ever reads its own: no barrier, no bank conflict); thread t owns the contiguous elements [8 t cpt, 8 (t + 1) cpt), cpt = ceil(V / 8 / 1024), so that a prefix over threads is a prefix in
// vocabulary order.  p is monotone in l, so K is a threshold on the order-preserving 16-bit key of the bf16 value: a bisection of at most
// 16 rounds of "mass of the keys >= t" over exp values kept in registers.  Every sum has a fixed order (per thread in index order, the
// wave's butterfly, the 16 wave partials in sequence; the scan: lanes in sequence, then waves in sequence): no atomics, a second launch
// on the same inputs is bit-identical.  temperature, top_p and u come from device memory: a captured graph serves every setting.
// sample_pick_kernel<true> (vrwkv_sample_pick_pen_bf16) is the same body on the row l' that the applications' occurrence counts make of l
// (VisualRWKV-v7/v7.10/app/app_gpu.py:56-86): the owner of a chunk reads its 2 x 16 bytes of occ while it turns the chunk into keys -- banned
// (c < 0): -inf; counted (c > 0): bf16(l - (alpha_presence + c alpha_count)), and c decay goes back -- and the winning thread, which owns the
// token's chunk, adds 1 to the token's count after its own decayed store.  Row b of occ is touched by workgroup b alone; no barrier is added.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/visualrwkv_hip.h"
#include <gfx950_prims.h>
#include "decode_common.h"
#include "host_checks.h"

namespace {

using namespace decode;

constexpr int SP_THREADS = 1024, SP_WAVES = SP_THREADS / 64;
constexpr int SP_MAXCH = 8;                                  // 8-element chunks per thread
constexpr int SP_MAXV = 8 * SP_THREADS * SP_MAXCH;           // 65 536
constexpr float SP_LOG2E = 1.4426950216293335f, SP_LOG2E_LO = 1.9259629911266175e-8f;       // log2(e) = hi + lo
constexpr float SP_NONE = 8388607.f;                         // "no candidate" of the index reduction (indices are below 2^17)

struct PickArgs {
    int V, C;
    const uint16_t* logits;
    const float *params, *u;
    const uint16_t* emb;
    uint16_t* x_out;
    int* token;
    float* logit_prob;
    float* occ;                                              // the penalised entry's counts; NULL in the plain one
};

enum { OP_SUM, OP_MAX, OP_MIN };
template <int OP> DEVFN float op(float a, float b) { return OP == OP_SUM ? a + b : OP == OP_MAX ? fmaxf(a, b) : fminf(a, b); }

// all-reduce over the workgroup in a fixed order; every thread gets the same bits
template <int OP> DEVFN float block_all(float x, float* red) {
    x = op<OP>(x, lane_xor1(x));
    x = op<OP>(x, lane_xor2(x));
    x = op<OP>(x, lane_half_mirror(x));
    x = op<OP>(x, lane_mirror(x));
    x = op<OP>(x, lane_xor16(x));
    x = op<OP>(x, lane_xor32(x));
    __syncthreads();                                     // red may still be read from the previous call
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    float r = red[0];
#pragma unroll
    for (int w = 1; w < SP_WAVES; ++w) r = op<OP>(r, red[w]);
    return r;
}

// two bf16 -> two keys whose unsigned order is the order of the values (sign clear: set the top bit; sign set: complement), and back
DEVFN uint32_t keys_of(uint32_t u) { return u ^ ((((u >> 15) & 0x00010001u) * 0xffffu) | 0x80008000u); }
DEVFN float value_of(uint32_t key) { return bf16_to_f32((uint16_t)((key & 0x8000u) ? key ^ 0x8000u : key ^ 0xffffu)); }
// exp2(x (c + c_lo)) for x <= 0 with the product split into its integer part and an exactly formed fraction: the relative error stays at the
// 1 ulp of v_exp_f32 whatever |x| (a plain exp2(x c) carries |x c| 2^-24 from the product's rounding: 45 ulp at x = -30).  x = -inf gives 0.
DEVFN float exp2_scaled(float x, float c, float c_lo) {
    x = fmaxf(x, -1000.f);
    const float n = rintf(x * c);
    return ldexpf(fast_exp2(fmaf(x, c, -n) + x * c_lo), (int)n);
}
DEVFN uint32_t key_at(const vrwkv_u4& k, int j) {
    const uint32_t w = j < 2 ? k.x : j < 4 ? k.y : j < 6 ? k.z : k.w;
    return (j & 1) ? w >> 16 : w & 0xffffu;
}

// One logit (bf16 bits) under the count c of its token: banned -> -inf; counted -> l - (alpha_presence + c alpha_count) rounded to bf16 as
// `out[n] -= ...` rounds on a bf16 tensor.  Product, sum and difference are each rounded on their own, as in torch.
DEVFN uint32_t penalised(uint32_t h, float c, float a_presence, float a_count) {
#pragma clang fp contract(off)
    if (c < 0.f) return 0xff80u;
    if (c > 0.f) {
        const float pen = a_presence + c * a_count;
        h = f32_to_bf16_bits(bf16_to_f32((uint16_t)h) - pen);
    }
    return h;
}
DEVFN uint32_t penalised2(uint32_t w, float c_lo, float c_hi, float a_presence, float a_count) {
    return penalised(w & 0xffffu, c_lo, a_presence, a_count) | (penalised(w >> 16, c_hi, a_presence, a_count) << 16);
}
DEVFN float decayed(float c, float decay) { return c > 0.f ? c * decay : c; }
// four counts after a pick; whether one of them changed (their 16 bytes go back only then)
DEVFN bool decay4(f32x4& o, float decay) {
    const bool any = o.x > 0.f || o.y > 0.f || o.z > 0.f || o.w > 0.f;
    o = f32x4{decayed(o.x, decay), decayed(o.y, decay), decayed(o.z, decay), decayed(o.w, decay)};
    return any;
}

template <bool PEN> __global__ __launch_bounds__(SP_THREADS) void sample_pick_kernel(PickArgs a) {
    __shared__ float red[SP_WAVES];
    __shared__ float wtot[SP_WAVES];
    __shared__ float tot[SP_THREADS];
    const int tid = threadIdx.x, lane = tid & 63, wave = uniform_i32(tid >> 6);
    const int b = blockIdx.x;
    const int nvec = a.V / 8, cpt = (nvec + SP_THREADS - 1) / SP_THREADS;
    const int c0 = tid * cpt;
    const uint16_t* row = a.logits + (size_t)b * a.V;
    const float temperature = a.params[0], top_p = a.params[1], u = a.u[b];
    // the row, as keys in LDS; a thread's chunks past the row hold the key of -inf (weight 0) and are kept out of K by `live`
    vrwkv_u4* const kl = reinterpret_cast<vrwkv_u4*>(dyn_lds()) + tid;          // chunk i of this thread: kl[i * SP_THREADS]
    const vrwkv_u4 dead = vrwkv_u4{0xff80ff80u, 0xff80ff80u, 0xff80ff80u, 0xff80ff80u};
    vrwkv_u4 raw[SP_MAXCH];
#pragma unroll
    for (int i = 0; i < SP_MAXCH; ++i) raw[i] = (i < cpt && c0 + i < nvec) ? ld16(row + (size_t)(c0 + i) * 8) : dead;
    // pass 1: the maximum, then e = exp(l - m) and Z
    uint32_t km = 0;
#pragma unroll
    for (int i = 0; i < SP_MAXCH; ++i) {
        if (i < cpt) {
            if constexpr (PEN) {
                if (c0 + i < nvec) {                         // the chunk's counts, consumed here: a second copy of the row in registers spills
                    f32x4* const oc = reinterpret_cast<f32x4*>(a.occ + (size_t)b * a.V + (size_t)(c0 + i) * 8);
                    f32x4 o0 = oc[0], o1 = oc[1];
                    const float ap = a.params[2], ac = a.params[3], decay = a.params[4];
                    raw[i] = vrwkv_u4{penalised2(raw[i].x, o0.x, o0.y, ap, ac), penalised2(raw[i].y, o0.z, o0.w, ap, ac),
                                      penalised2(raw[i].z, o1.x, o1.y, ap, ac), penalised2(raw[i].w, o1.z, o1.w, ap, ac)};
                    if (decay4(o0, decay)) oc[0] = o0;
                    if (decay4(o1, decay)) oc[1] = o1;
                }
            }
            const vrwkv_u4 k = vrwkv_u4{keys_of(raw[i].x), keys_of(raw[i].y), keys_of(raw[i].z), keys_of(raw[i].w)};
            kl[i * SP_THREADS] = k;
#pragma unroll
            for (int j = 0; j < 8; ++j) { const uint32_t kj = key_at(k, j); km = kj > km ? kj : km; }
        }
    }
    const uint32_t kmax = (uint32_t)block_all<OP_MAX>((float)km, red);      // keys are below 2^16: exact as floats
    const float m = value_of(kmax);
    float e[SP_MAXCH][8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < SP_MAXCH; ++i) {
        if (i < cpt) {
            const vrwkv_u4 k = kl[i * SP_THREADS];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                e[i][j] = exp2_scaled(value_of(key_at(k, j)) - m, SP_LOG2E, SP_LOG2E_LO);
                s += e[i][j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) e[i][j] = 0.f;
        }
    }
    const float Z = block_all<OP_SUM>(s, red);
    // pass 2: the largest key t with mass(keys >= t) >= top_p Z.  mass(0) = Z and mass(kmax) > 0 hold by construction: top_p >= 1
    // keeps every token, top_p = 0 the maximum and its ties.
    const float P = top_p * Z;
    uint32_t lo = 0, hi = top_p >= 1.f ? 1u : kmax + 1u;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        float ms = 0.f;
#pragma unroll
        for (int i = 0; i < SP_MAXCH; ++i) {
            if (i < cpt) {
                const vrwkv_u4 k = kl[i * SP_THREADS];
#pragma unroll
                for (int j = 0; j < 8; ++j) ms += key_at(k, j) >= mid ? e[i][j] : 0.f;
            }
        }
        if (block_all<OP_SUM>(ms, red) >= P) lo = mid; else hi = mid;
    }
    const uint32_t thr = lo;
    // pass 3: q = exp((l - m) / temperature) on K (0 elsewhere), per-thread totals, their exclusive scan in thread order
    const float sc = SP_LOG2E / temperature;
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < SP_MAXCH; ++i) {
        if (i < cpt) {
            const bool live = c0 + i < nvec;
            const vrwkv_u4 k = kl[i * SP_THREADS];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint32_t kj = key_at(k, j);
                e[i][j] = (live && kj >= thr) ? exp2_scaled(value_of(kj) - m, sc, 0.f) : 0.f;
                t += e[i][j];
            }
        }
    }
    tot[tid] = t;
    __syncthreads();
    float lp = 0.f;                                      // the lanes before this one, in lane order
    for (int j = 0; j < 64; ++j) { const float v = tot[wave * 64 + j]; lp += j < lane ? v : 0.f; }
    if (lane == 63) wtot[wave] = lp + t;
    __syncthreads();
    float wp = 0.f, total = 0.f;                         // the waves before this one, and all of them, in wave order
#pragma unroll
    for (int w = 0; w < SP_WAVES; ++w) { if (w == wave) wp = total; total += wtot[w]; }
    // pass 4: the first member of K (of weight > 0) whose running sum exceeds u total; failing that (rounding) the last such member
    const float target = u * total;
    float acc = wp + lp;
    int cand = -1, last = -1;
    uint32_t ckey = 0, lkey = 0;
#pragma unroll
    for (int i = 0; i < SP_MAXCH; ++i) {
        if (i < cpt) {
            const vrwkv_u4 k = kl[i * SP_THREADS];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float q = e[i][j];
                acc += q;
                if (q > 0.f) {
                    const int idx = (c0 + i) * 8 + j;
                    const uint32_t kj = key_at(k, j);
                    if (acc > target && cand < 0) { cand = idx; ckey = kj; }
                    last = idx; lkey = kj;
                }
            }
        }
    }
    const float code = cand >= 0 ? (float)cand : last >= 0 ? (float)(2 * SP_MAXV - 1 - last) : SP_NONE;
    const int win = (int)block_all<OP_MIN>(code, red);
    int token = 0;
    bool mine = false;
    uint32_t wkey = 0;
    if (win < SP_MAXV) { token = win; mine = cand == win; wkey = ckey; }
    else if (win < 2 * SP_MAXV) { token = 2 * SP_MAXV - 1 - win; mine = cand < 0 && last == token; wkey = lkey; }
    else mine = tid == 0;                                // no weight anywhere (a row the contract leaves undefined): token 0, NaN beside it
    if (mine) {
        const float l = win < 2 * SP_MAXV ? value_of(wkey) : __uint_as_float(0x7fc00000u);
        a.token[b] = token;
        a.logit_prob[2 * b] = l;
        a.logit_prob[2 * b + 1] = exp2_scaled(l - m, SP_LOG2E, SP_LOG2E_LO) / Z;
        if constexpr (PEN) {
            if (win < 2 * SP_MAXV) {                         // this thread owns the token's chunk: the read follows its own decayed store
                f32x4* const oc = reinterpret_cast<f32x4*>(a.occ + (size_t)b * a.V + (size_t)(token & ~3));
                f32x4 o = *oc;
                o[token & 3] += 1.f;
                *oc = o;
            }
        }
    }
    if (a.emb) {
        const uint16_t* src = a.emb + (size_t)token * a.C;
        uint16_t* dst = a.x_out + (size_t)b * a.C;
        for (int c = tid; c < a.C / 8; c += SP_THREADS) *reinterpret_cast<vrwkv_u4*>(dst + c * 8) = ld16(src + c * 8);
    }
}

inline bool off4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; }

// both entries: the checks in the order count, shape, NULL, alignment, then the launch
int pick_entry(bool pen, int B, int V, int C, const void* logits, const float* params, const float* u, float* occ, const void* emb, void* x_out,
               int* token, float* logit_prob, void* stream) {
    if (B <= 0) return VRWKV_EINVAL;
    if (V <= 0 || V % 8 != 0 || V > SP_MAXV || C <= 0 || C % 8 != 0) return VRWKV_ESHAPE;
    if (hostchk::any_null(logits, params, u, token, logit_prob) || (pen && occ == nullptr) || (emb == nullptr) != (x_out == nullptr))
        return VRWKV_EINVAL;
    // the row, its counts, the embedding and x_out move in 16-byte pieces; the scalars by element
    if (hostchk::any_misaligned(logits, occ, emb, x_out) || off4(params) || off4(u) || off4(token) || off4(logit_prob)) return VRWKV_EALIGN;
    PickArgs a{};
    a.V = V; a.C = C; a.logits = (const uint16_t*)logits; a.params = params; a.u = u;
    a.emb = (const uint16_t*)emb; a.x_out = (uint16_t*)x_out; a.token = token; a.logit_prob = logit_prob; a.occ = occ;
    const size_t lds = (size_t)((V / 8 + SP_THREADS - 1) / SP_THREADS) * SP_THREADS * 16;      // the row's keys: up to 128 KB
    return hostchk::launch_lds(pen ? sample_pick_kernel<true> : sample_pick_kernel<false>, dim3((unsigned)B), dim3(SP_THREADS), lds,
                               (hipStream_t)stream, a);
}

}  // namespace

extern "C" int vrwkv_sample_pick_bf16(int B, int V, int C, const void* logits, const float* params, const float* u, const void* emb,
                                      void* x_out, int* token, float* logit_prob, void* stream) {
    return pick_entry(false, B, V, C, logits, params, u, nullptr, emb, x_out, token, logit_prob, stream);
}

extern "C" int vrwkv_sample_pick_pen_bf16(int B, int V, int C, const void* logits, const float* params, const float* u, float* occ,
                                          const void* emb, void* x_out, int* token, float* logit_prob, void* stream) {
    return pick_entry(true, B, V, C, logits, params, u, occ, emb, x_out, token, logit_prob, stream);
}
