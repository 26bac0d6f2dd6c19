// Host launchers + C-ABI for the WKV7 kernels (include/visualrwkv_hip.h).  The profiling entry point is wkv7_profile.hip; A/B partners
// that are not part of the product (wkv7_bwd_v7.h, builds with one or two wave roles switched off, the tail on the J waves) come in
// through benchmarks/experiments/wkv7_experiments.h when the library is built with -DVRWKV_V6_EXPERIMENTS (benchmarks/build_alt.sh).
#include <atomic>
#include <wkv7_launch.h>
#include <wkv7_chunked.h>
#include <wkv7_fwd_v3.h>
#include <wkv7_fwd_v4.h>
#include <wkv7_bwd_v5.h>
#include <wkv7_bwd_v6.h>     // shared building blocks of the backward kernels
#include <wkv7_bwd_v8.h>
#ifdef VRWKV_V6_EXPERIMENTS
#include <wkv7_experiments.h>
#endif

namespace wkv7launch {
std::atomic<int> g_fwd_variant{-1}, g_bwd_variant{-1};
}

namespace {
using namespace wkv7launch;
// what the last launch of each direction resolved to (vrwkv_wkv7_last_variant): a single-threaded test aid -- launches come from the
// Python thread AND from autograd's backward thread, so code that needs to know which kernel a launch of a given shape uses asks
// vrwkv_wkv7_resolve_variant (a pure function of the shape and the override) instead of reading this after the fact
std::atomic<int> g_last_fwd{0}, g_last_bwd{0};
// The instantiations the library launches.  Where an instantiation is first mentioned decides where it lies in the code object: the order of this
// list -- forward, backward plain and state, then the packed ones -- is the layout the code object has had, so keep it and add at the end.
using FwdKernel = void (*)(wkv7::FwdArgs);
using BwdKernel = void (*)(wkv7::BwdArgs);
constexpr FwdKernel FWD_FULL_ROW = &wkv7f4::fwd_kernel_v4<false>;        // 7: full-row memory traffic (wkv7_fwd_v4.h)
// Chunked MFMA, producer / consumer waves (wkv7_fwd_v3.h), by variant; [0] and [4] are the default instantiation: no Ab / Kb images (state update
// from Ah / Kh, scaled by c_L afterwards; T chain splitting every matrix once per level) + natural [t][j] images read with ds_read_b64_tr_b16.
// Same-box A/B (benchmarks/wkv7_ab.py --fwd 1 2 4): B=8 0.358 -> 0.331 -> 0.324 ms, B=16 0.647 -> 0.637 -> 0.627 ms.
constexpr FwdKernel FWD_CHUNKED[7] = {
    &wkv7c::fwd_kernel_v3<false, false, 1, 1, false, true, true>,
    &wkv7c::fwd_kernel_v3<false, false, 1>,                                  // 1: the round-2 instantiation
    &wkv7c::fwd_kernel_v3<false, false, 1, 1, false, false, true>,           // 2
    &wkv7c::fwd_kernel_v3<false, true, 1, 1, false, false, true>,            // 3: + 16-byte transposed stores
    &wkv7c::fwd_kernel_v3<false, false, 1, 1, false, true, true>,            // 4
    &wkv7c::fwd_kernel_v3<false, false, 1, 2, false, false, true>,           // 5: + two chunks of prefetch
    &wkv7c::fwd_kernel_v3<false, false, 1, 1, false, true, true, true>};     // 6: two workgroups per head
// backward: 5 = wkv7_bwd_v5.h (8 waves; also the sequence-parallel kernel), 8 = wkv7_bwd_v8.h (one dS copy, T chain on P wave 0, full-row LDS-DMA),
// 9 = 8 with the score pieces a step ahead on the P waves.  (6 = the round-3 kernel, experiment builds only: benchmarks/experiments/wkv7_bwd_v6_kernel.h)
constexpr int BWD_DEFAULT = 9;
// {9, 8, 5} of the plain entry, of the state entry (5: the sequence-parallel kernel with one segment per head, which carries both state gradients
// already), then the packed forward and {9, 8} of the packed backward (wkv7_bwd_v5.h has no resets)
constexpr BwdKernel BWD_PLAIN[3] = {&wkv7v8::bwd_kernel_v8<false, true>, &wkv7v8::bwd_kernel_v8<false>, &wkv7v5::bwd_kernel_v5<false, BWD_V5_MODE>};
constexpr BwdKernel BWD_STATE[3] = {&wkv7v8::bwd_kernel_v8<false, true, true>, &wkv7v8::bwd_kernel_v8<false, false, true>, &wkv7v5::bwd_kernel_v5<false, BWD_V5_MODE, true>};
constexpr FwdKernel FWD_FULL_ROW_PACKED = &wkv7f4::fwd_kernel_v4<false, 1, true>;
constexpr BwdKernel BWD_PACKED[2] = {&wkv7v8::bwd_kernel_v8<false, true, false, true>, &wkv7v8::bwd_kernel_v8<false, false, false, true>};
// wkv7_bwd_v8.h forms 32-bit byte offsets inside a tensor (the largest is the fp32 `sa`): a launch whose tensors reach this many bytes is cut into
// batch slices below it (every tensor of the op is batch-major, so a slice is the same launch on offset pointers); a single sample that large goes
// to wkv7_bwd_v5.h, which addresses with 64 bits.  vrwkv_wkv7_set_backward_slice_limit lowers it for tests.
std::atomic<unsigned long long> g_slice_limit{1ull << 32};

// The kernel a forward launch of `heads` = B x H workgroups uses under override `forced` (-1: none): 7 = wkv7_fwd_v4.h (full-row memory traffic)
// when the heads alone give every CU a workgroup pair's worth of work, 6 = wkv7_fwd_v3.h with two workgroups per head below that, else the forced
// instantiation of wkv7_fwd_v3.h.  The stateful entry (vrwkv_wkv7_forward_state_bf16) follows the same rule; its A/B overrides 1..5 all mean 4
// (the default instantiation of wkv7_fwd_v3.h: the others have no state arguments).
int resolve_fwd(long heads, int forced, bool stateful) {
    if (forced == 7 || (forced == -1 && heads > FWD_ISPLIT_MAX_HEADS)) return 7;
    if (forced == -1 || forced == 6) return 6;
    return stateful ? 4 : forced;
}
// backward: variant 9 when the launch has more workgroups than the chip has CUs (measured -0.4 ... -2.3 % at B x H = 384 ... 1024), variant 8
// for a single round of workgroups (B x H <= 256: 9 measured +0.3 ... +1.8 % there); profiles/r4_wkv7_ab.jsonl, r4c_wkv7_ab.jsonl
int resolve_bwd(long heads, int forced) { return forced == -1 ? (heads > 256 ? BWD_DEFAULT : 8) : forced; }

enum class Fwd { plain, state, packed };      // what a forward entry asks of the by-products: both, any, both or neither
// Every forward entry: checks (sizes, then NULL pointers, then alignment), kernel choice, record, launch.
int fwd_launch(Fwd kind, int B, int T, int H, const wkv7::FwdArgs& p, void* stream) {
    if (int rc = check_common(B, T, H)) return rc;
    if (any_null(p.w, p.q, p.k, p.v, p.z, p.a, p.y)) return VRWKV_EINVAL;
    // plain: s and sa are outputs of the op; packed: optional, together; state: optional, each on its own
    if (kind == Fwd::plain ? (!p.s || !p.sa) : (kind == Fwd::packed && !p.s != !p.sa)) return VRWKV_EINVAL;
    if (any_misaligned(p.w, p.q, p.k, p.v, p.z, p.a, p.y, p.s, p.sa, p.s0, p.s_final)) return VRWKV_EALIGN;      // NULL passes: the optional ones go with the rest
    const long heads = (long)B * H;
    // packed rows: the full-row kernel at every size and under every override (it runs at any number of heads; the two-workgroups-per-head
    // form of wkv7_fwd_v3.h has no resets).  state: resolve_fwd turns the overrides 1..5 into 4, so only 4, 6 and 7 reach the choice below.
    const int var = kind == Fwd::packed ? 7 : resolve_fwd(heads, g_fwd_variant.load(), kind == Fwd::state);
    g_last_fwd = var;
    hipStream_t st = (hipStream_t)stream;
    if (var == 7)        // it takes the state arguments and skips the by-products it has no buffers for
        return launch_lds(p.chunk_reset ? FWD_FULL_ROW_PACKED : FWD_FULL_ROW, dim3((unsigned)heads), dim3(512), sizeof(wkv7f4::LdsF4), st, p);
    return launch_lds(FWD_CHUNKED[var], dim3((unsigned)(var == 6 ? 2 * heads : heads)), dim3(512), sizeof(wkv7c::LdsF), st, p);
}

// The checks of every backward entry, in this order: sizes, NULL among the required pointers, nseg (the segments entry; 1 elsewhere, which
// passes), alignment.  NULL is not misaligned, so the optional pointers are checked with the rest.
int bwd_check(int B, int T, int H, const BwdCall& c) {
    if (int rc = check_common(B, T, H)) return rc;
    if (any_null(c.w, c.q, c.k, c.v, c.z, c.a, c.dy, c.s, c.sa, c.dw, c.dq, c.dk, c.dv, c.dz, c.da)) return VRWKV_EINVAL;
    if (c.nseg < 1 || c.nseg > T / VRWKV_CHUNK_LEN) return VRWKV_ESHAPE;
    if (any_misaligned(c.w, c.q, c.k, c.v, c.z, c.a, c.dy, c.s, c.sa, c.dw, c.dq, c.dk, c.dv, c.dz, c.da, c.s0, c.ds_final, c.ds0)) return VRWKV_EALIGN;
    return VRWKV_OK;
}

// The instantiation behind variant `var` (9, 8, else 5) of the plain, the state and the packed entry.
BwdKernel bwd_kernel(int var, bool state, bool packed) {
    return (packed ? BWD_PACKED : state ? BWD_STATE : BWD_PLAIN)[var == 9 ? 0 : var == 8 ? 1 : 2];
}

// The plain, state and packed backward entries: checks, kernel choice, batch slices, record, one launch per slice.
int bwd_launch(int B, int T, int H, const BwdCall& c, void* stream) {
    if (int rc = bwd_check(B, T, H, c)) return rc;
    const bool packed = c.chunk_reset != nullptr;
    int var = resolve_bwd((long)B * H, g_bwd_variant.load());
    bool v8 = var == 8 || var == 9;                  // wkv7_bwd_v8.h, the only kernel that is sliced; else 5 or, in the plain entry, an experiment variant
    if (c.state && !v8) var = 5;                     // state: every other variant is wkv7_bwd_v5.h's sequence-parallel kernel, nseg = 1
    if (packed && !v8) return VRWKV_ESHAPE;          // packed: wkv7_bwd_v5.h has no resets, the caller runs the samples one by one; nothing is recorded
    // batch slices for the 32-bit offsets of wkv7_bwd_v8.h (see g_slice_limit)
    const unsigned long long per_sample = (unsigned long long)T * H * 64ull * 4ull, limit = g_slice_limit.load();
    int bmax = B;
    if (v8 && (unsigned long long)B * per_sample >= limit) {
        bmax = (int)((limit - 1) / per_sample);
        if (bmax < 1) {                              // a single sample at or above the limit: wkv7_bwd_v5.h unsliced; packed: as above
            if (packed) return VRWKV_ESHAPE;
            var = 5; bmax = B; v8 = false;
        }
    }
    g_last_bwd = var;
    for (int b0 = 0; b0 < B; b0 += bmax) {
        const wkv7::BwdArgs p = bwd_args(c, T, H, b0);
        const dim3 grid((unsigned)((long)(B - b0 < bmax ? B - b0 : bmax) * H));
        int rc;
#ifdef VRWKV_V6_EXPERIMENTS
        if (wkv7exp::is_experiment(var)) rc = wkv7exp::launch(var, grid, (hipStream_t)stream, p); else      // the plain entry only: state has made them 5, packed has returned
#endif
        rc = launch_lds(bwd_kernel(var, c.state, packed), grid, dim3(v8 ? 768 : 512), v8 ? sizeof(wkv7v8::LdsV8) : sizeof(wkv7v5::LdsV5), (hipStream_t)stream, p);
        if (rc) return rc;
    }
    return VRWKV_OK;
}
}  // namespace

extern "C" {

int vrwkv_abi_version(void) { return 1; }

const char* vrwkv_strerror(int code) {
    switch (code) {
        case VRWKV_OK: return "ok";
        case VRWKV_EINVAL: return "invalid argument (null pointer or non-positive size)";
        case VRWKV_ESHAPE: return "T must be a multiple of 16";
        case VRWKV_EALIGN: return "pointer not 16-byte aligned";
        default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown error";
    }
}

int vrwkv_wkv7_set_forward_variant(int variant) {
    if (variant != -1 && !(variant >= 1 && variant <= 7)) return VRWKV_EINVAL;   // 1..5: A/B instantiations of wkv7_fwd_v3.h; 6: its two-workgroups-per-head form; 7: wkv7_fwd_v4.h
    g_fwd_variant = variant;
    return VRWKV_OK;
}

int vrwkv_wkv7_set_backward_variant(int variant) {
    bool ok = variant == -1 || variant == 5 || variant == 8 || variant == 9;      // see include/visualrwkv_hip.h
#ifdef VRWKV_V6_EXPERIMENTS
    ok = ok || wkv7exp::is_experiment(variant);
#endif
    if (!ok) return VRWKV_EINVAL;
    g_bwd_variant = variant;
    return VRWKV_OK;
}

int vrwkv_wkv7_set_backward_slice_limit(unsigned long long bytes) {
    g_slice_limit = bytes ? bytes : (1ull << 32);
    return VRWKV_OK;
}

int vrwkv_wkv7_last_variant(int backward) { return backward ? g_last_bwd.load() : g_last_fwd.load(); }

int vrwkv_wkv7_resolve_variant(int kind, int B, int T, int H) {
    if (check_common(B, T, H) != VRWKV_OK || kind < 0 || kind > 5) return VRWKV_EINVAL;
    const long heads = (long)B * H;
    if (kind == 1 || kind == 3 || kind == 5) return resolve_bwd(heads, g_bwd_variant.load());
    if (kind == 4) return 7;       // packed rows: wkv7_fwd_v4.h at every size
    return resolve_fwd(heads, g_fwd_variant.load(), kind == 2);
}

int vrwkv_wkv7_forward_bf16(int B, int T, int H, const void* w, const void* q, const void* k, const void* v,
                            const void* z, const void* a, void* y, float* s, float* sa, void* stream) {
    return fwd_launch(Fwd::plain, B, T, H, fwd_args(T, H, w, q, k, v, z, a, y, s, sa), stream);
}

int vrwkv_wkv7_forward_state_bf16(int B, int T, int H, const void* w, const void* q, const void* k, const void* v,
                                  const void* z, const void* a, void* y, const float* s0, float* s_final, float* s_ckpt,
                                  float* sa, void* stream) {
    wkv7::FwdArgs p = fwd_args(T, H, w, q, k, v, z, a, y, s_ckpt, sa);
    p.s0 = s0; p.s_final = s_final;
    return fwd_launch(Fwd::state, B, T, H, p, stream);
}

int vrwkv_wkv7_forward_packed_bf16(int B, int T, int H, const void* w, const void* q, const void* k, const void* v,
                                   const void* z, const void* a, void* y, const unsigned char* chunk_reset,
                                   float* s_ckpt, float* sa, void* stream) {
    wkv7::FwdArgs p = fwd_args(T, H, w, q, k, v, z, a, y, s_ckpt, sa);
    p.chunk_reset = chunk_reset;
    return fwd_launch(Fwd::packed, B, T, H, p, stream);
}

int vrwkv_wkv7_backward_bf16(int B, int T, int H, const void* w, const void* q, const void* k, const void* v,
                             const void* z, const void* a, const void* dy, const float* s, const float* sa,
                             void* dw, void* dq, void* dk, void* dv, void* dz, void* da, void* stream) {
    return bwd_launch(B, T, H, BwdCall{w, q, k, v, z, a, dy, s, sa, dw, dq, dk, dv, dz, da}, stream);
}

int vrwkv_wkv7_backward_state_bf16(int B, int T, int H, const void* w, const void* q, const void* k, const void* v,
                                   const void* z, const void* a, const void* dy, const float* s, const float* sa,
                                   const float* s0, const float* ds_final, float* ds0,
                                   void* dw, void* dq, void* dk, void* dv, void* dz, void* da, void* stream) {
    BwdCall c{w, q, k, v, z, a, dy, s, sa, dw, dq, dk, dv, dz, da, s0, ds_final, ds0};
    c.state = true;
    return bwd_launch(B, T, H, c, stream);
}

// chunk_reset == NULL is the plain entry
int vrwkv_wkv7_backward_packed_bf16(int B, int T, int H, const void* w, const void* q, const void* k, const void* v,
                                    const void* z, const void* a, const void* dy, const float* s, const float* sa,
                                    const unsigned char* chunk_reset,
                                    void* dw, void* dq, void* dk, void* dv, void* dz, void* da, void* stream) {
    BwdCall c{w, q, k, v, z, a, dy, s, sa, dw, dq, dk, dv, dz, da};
    c.chunk_reset = chunk_reset;
    return bwd_launch(B, T, H, c, stream);
}

// nseg workgroups per head, no batch slices (wkv7_bwd_v5.h addresses with 64 bits), nothing recorded
int vrwkv_wkv7_backward_segments_bf16(int B, int T, int H, int nseg, const void* w, const void* q, const void* k, const void* v,
                                      const void* z, const void* a, const void* dy, const float* s, const float* sa,
                                      const float* ds_in, float* ds_out,
                                      void* dw, void* dq, void* dk, void* dv, void* dz, void* da, void* stream) {
    BwdCall c{w, q, k, v, z, a, dy, s, sa, dw, dq, dk, dv, dz, da, nullptr, ds_in, ds_out};
    c.nseg = nseg;
    if (int rc = bwd_check(B, T, H, c)) return rc;
    return launch_lds(&wkv7v5::bwd_kernel_v5<false, BWD_V5_MODE, true>, dim3((unsigned)((long)B * H * nseg)), dim3(512), sizeof(wkv7v5::LdsV5),
                      (hipStream_t)stream, bwd_args(c, T, H));
}

}  // extern "C"
