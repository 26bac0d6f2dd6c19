// State and helpers shared by the WKV7 launchers (wkv7_capi.hip) and the profiling entry point (wkv7_profile.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>

#include "../../include/visualrwkv_hip.h"
#include <host_checks.h>
#include <wkv7_kernels.h>

namespace wkv7launch {

extern std::atomic<int> g_fwd_variant, g_bwd_variant;      // vrwkv_wkv7_set_{forward,backward}_variant; -1 = default
// few heads (B*H <= 128: at most half of the 256 CUs would be busy): the forward runs two workgroups per head, 32 value rows each
constexpr long FWD_ISPLIT_MAX_HEADS = 128;
// T chain on the bf16 matrix core (2) + producer priority 2 (4; same-box A/B: 1.18 -> 1.09 ms) + priorities swapped in
// segment 1, where the producers have ~1.2k cycles of slack per chunk and the consumers none (128; 1.09 -> 1.04 ms)
constexpr int BWD_V5_MODE = 2 + 4 + 128;

using hostchk::any_misaligned;
using hostchk::any_null;
using hostchk::finish_launch;
using hostchk::launch_lds;
using hostchk::misaligned;
inline int check_common(int B, int T, int H) {
    if (B <= 0 || T <= 0 || H <= 0) return VRWKV_EINVAL;
    if (T % VRWKV_CHUNK_LEN != 0) return VRWKV_ESHAPE;   // cuda_backward asserts this, wkv7_cuda.cu:136
    return VRWKV_OK;
}

// The argument block of a forward launch from the tensors every forward entry takes; s0, s_final, chunk_reset and dbg are set by the entry that has them.
inline wkv7::FwdArgs fwd_args(int T, int H, const void* w, const void* q, const void* k, const void* v, const void* z, const void* a,
                              void* y, float* s, float* sa) {
    return wkv7::FwdArgs{T, H, (const uint16_t*)w, (const uint16_t*)q, (const uint16_t*)k, (const uint16_t*)v,
                         (const uint16_t*)z, (const uint16_t*)a, (uint16_t*)y, s, sa};
}

// The tensors of a backward launch as the C entries receive them (whole batch).
struct BwdCall {
    const void *w, *q, *k, *v, *z, *a, *dy;           // bf16 (B,T,H,64)
    const float *s, *sa;                              // the forward's by-products
    void *dw, *dq, *dk, *dv, *dz, *da;                // bf16 (B,T,H,64)
    // optional.  Carried state: s0 / ds_final / ds0, (B,H,64,64).  Segments (never sliced): ds_final / ds0 are its ds_in / ds_out, (B,H,nseg,64,64)
    const float *s0 = nullptr, *ds_final = nullptr;
    float* ds0 = nullptr;
    const unsigned char* chunk_reset = nullptr;       // packed rows: (B,T/16)
    int nseg = 1;
    bool state = false;                               // the state entry: six gradients wanted whatever ds_final / ds0 are
    unsigned long long* dbg = nullptr;                // profiling builds
};

// The argument block of the batch slice that begins at sample b0: every tensor is batch-major, so a slice is the same launch on offset pointers.
inline wkv7::BwdArgs bwd_args(const BwdCall& c, int T, int H, int b0 = 0) {
    const size_t nc = (size_t)(T / VRWKV_CHUNK_LEN);
    const size_t o = (size_t)b0 * T * H * 64, ckpt = (size_t)b0 * H * nc * 64 * 64, stt = (size_t)b0 * H * 64 * 64;      // elements
    wkv7::BwdArgs p{T, H, (const uint16_t*)c.w + o, (const uint16_t*)c.q + o, (const uint16_t*)c.k + o, (const uint16_t*)c.v + o,
                    (const uint16_t*)c.z + o, (const uint16_t*)c.a + o, (const uint16_t*)c.dy + o, c.s + ckpt, c.sa + o,
                    (uint16_t*)c.dw + o, (uint16_t*)c.dq + o, (uint16_t*)c.dk + o, (uint16_t*)c.dv + o, (uint16_t*)c.dz + o, (uint16_t*)c.da + o, c.dbg};
    p.ds_in = c.ds_final ? c.ds_final + stt : nullptr;
    p.ds_out = c.ds0 ? c.ds0 + stt : nullptr;
    p.s0 = c.s0 ? c.s0 + stt : nullptr;
    p.nseg = c.nseg;
    p.want_grads = c.state;
    p.chunk_reset = c.chunk_reset ? c.chunk_reset + (size_t)b0 * nc : nullptr;
    return p;
}

}  // namespace wkv7launch
