// WKV7 ("wind_backstepping") operator for gfx950: shared constants and the argument blocks of the kernels.
//
// Math (reference: VisualRWKV-v7/v7.00/cuda/wkv7_cuda.cu:10-130), per (b,h),
// S in R^{64x64}, rows i = value index, columns j = key index, w_t = exp(-exp(w_raw_t)):
//     sa_t = S_{t-1} z_t ;  S_t = S_{t-1} diag(w_t) + sa_t a_t^T + v_t k_t^T ;  y_t = S_t q_t
// (argument names follow the op schema: z = -kk, a = kk*gate).
// The kernels: wkv7_fwd_v3.h (forward), wkv7_bwd_v6.h (backward), wkv7_bwd_v5.h (sequence-parallel backward and the
// shared backward building blocks), wkv7_step.hip (single-token step).  The first generation (sequential in T, one wave per
// head, VALU formulation: 15-33 % / 8-11 % of the HBM roofline) and the first producer / consumer backward were removed
// from the library in round 3; DESIGN.md section 3.1 keeps their measurements.
#pragma once
#include <gfx950_prims.h>

namespace wkv7 {

constexpr int N = 64;        // head size (RUN_CUDA_RWKV7g hard-codes 64, src/model.py:69)
constexpr int CHUNK = 16;    // checkpoint interval of `s` (CHUNK_LEN, src/model.py:41)

template <int X> struct Log2 { static constexpr int v = 1 + Log2<X / 2>::v; };
template <> struct Log2<1> { static constexpr int v = 0; };

struct FwdArgs {
    int T, H;
    const uint16_t *w, *q, *k, *v, *z, *a;   // bf16 (B,T,H,N)
    uint16_t* y;                             // bf16 (B,T,H,N)
    float* s;                                // f32 (B,H,T/16,N,N)  holds S^T at chunk ends
    float* sa;                               // f32 (B,T,H,N)
    unsigned long long* dbg = nullptr;       // optional: per-phase cycle counts of workgroup 0 (profiling builds)
    // inference / stateful extensions honoured by fwd_kernel_v3 only (s and sa may then be null = not written):
    const float* s0 = nullptr;               // f32 (B,H,N,N) initial state S[i][j] (i = value row, j = key column)
    float* s_final = nullptr;                // f32 (B,H,N,N) state after the last token, same layout
    // packed rows (fwd_kernel_v4<.., PACKED> only): (B, T/16) bytes; non-zero = this chunk starts a new sample, from S = 0
    const unsigned char* chunk_reset = nullptr;
};

// ------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------
struct BwdArgs {
    int T, H;
    const uint16_t *w, *q, *k, *v, *z, *a, *dy;   // bf16 (B,T,H,N)
    const float* s;                               // f32 (B,H,T/16,N,N)
    const float* sa;                              // f32 (B,T,H,N)
    uint16_t *dw, *dq, *dk, *dv, *dz, *da;        // bf16 (B,T,H,N)
    unsigned long long* dbg = nullptr;
    // sequence-parallel backward (bwd_kernel_v3<.., TPAR = true>): nseg workgroups per head, each walks a contiguous range
    // of chunks from ds_in[b,h,seg] (dL/dS at the END of its range; null = 0) and leaves dL/dS at the START in ds_out
    const float* ds_in = nullptr;                 // f32 (B,H,nseg,N,N), [i][j]
    float* ds_out = nullptr;
    int nseg = 1;
    // carried state (bwd_kernel_v8<.., STATE>, bwd_kernel_v5<.., TPAR> with nseg = 1): the state the forward started from, [i][j] like ds_in
    // (null = 0).  The checkpoints `s` begin at the END of chunk 0, so the j-split of chunk 0 (dq, dz and through them dw) takes its S0 from here.
    const float* s0 = nullptr;                    // f32 (B,H,N,N)
    int want_grads = 0;                           // TPAR: 1 = a launch with ds_out and no ds_in still computes the six gradients (the state op);
                                                  // 0 = it is pass 1 of the sequence-parallel backward, whose gradients nobody reads (LITE)
    // packed rows (bwd_kernel_v8<.., PACKED> only): (B, T/16) bytes, as FwdArgs::chunk_reset; `s` is then the walk WITH the resets
    const unsigned char* chunk_reset = nullptr;
};

// One byte of a flag array at a wave-uniform index, as a scalar: the aligned dword that holds it comes through the constant address space
// (s_load_dword: counted by lgkmcnt, so it neither waits for nor disturbs the vector-memory counter the memory roles of the kernels count
// by hand), the byte is shifted out on the scalar unit.  The load covers the aligned 4-byte granule around the byte: up to 3 bytes before
// the first / after the last flag of the array are read (never used), which every device allocation contains.
DEVFN unsigned uniform_flag_u8(const unsigned char* flags, int idx) {
#if defined(__HIP_DEVICE_COMPILE__)
    const unsigned long long a = (unsigned long long)(uintptr_t)(flags + idx);
    typedef __attribute__((address_space(4))) const unsigned* const_u32_ptr;
    const unsigned word = *(const_u32_ptr)(a & ~3ull);
    return __builtin_amdgcn_readfirstlane((word >> (8u * ((unsigned)a & 3u))) & 0xffu);
#else
    return flags[idx];
#endif
}


}  // namespace wkv7
