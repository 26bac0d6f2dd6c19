// The PACKED instantiations of wkv7_fwd_v4.h and wkv7_bwd_v8.h (several samples end to end in a row: the state and dL/dS reset at flagged
// chunks) under the host lockstep emulator.  TEST INFRASTRUCTURE ONLY -- the C entries on top of them (vrwkv_wkv7_forward_packed_bf16,
// vrwkv_wkv7_backward_packed_bf16) come in through emu_wkv7_capi.cpp.
#include <gfx950_prims.h>   // resolves to tests/emu/gfx950_prims.h (-I order)
#include <wkv7_kernels.h>
#include <wkv7_chunked.h>
#include <wkv7_fwd_v4.h>
#include <wkv7_bwd_v6.h>
#include <wkv7_bwd_v8.h>

extern "C" int emu_wkv7_forward_packed_v4(int B, int T, int H, const void* w, const void* q, const void* k, const void* v, const void* z,
                                          const void* a, void* y, const unsigned char* chunk_reset, float* s_ckpt, float* sa) {
    wkv7::FwdArgs p{T, H, (const uint16_t*)w, (const uint16_t*)q, (const uint16_t*)k, (const uint16_t*)v,
                    (const uint16_t*)z, (const uint16_t*)a, (uint16_t*)y, s_ckpt, sa};
    p.chunk_reset = chunk_reset;
    const dim3 grid((unsigned)(B * H));
    if (chunk_reset) emu::launch(grid, dim3(512), [&] { wkv7f4::fwd_kernel_v4<false, 1, true>(p); });
    else emu::launch(grid, dim3(512), [&] { wkv7f4::fwd_kernel_v4<false>(p); });
    return (int)sizeof(wkv7f4::LdsF4);
}

extern "C" int emu_wkv7_backward_packed_v8(int B, int T, int H, const void* w, const void* q, const void* k, const void* v,
                                           const void* z, const void* a, const void* dy, const float* s, const float* sa,
                                           const unsigned char* chunk_reset,
                                           void* dw, void* dq, void* dk, void* dv, void* dz, void* da, int ahead) {
    wkv7::BwdArgs p{T, H, (const uint16_t*)w, (const uint16_t*)q, (const uint16_t*)k, (const uint16_t*)v,
                    (const uint16_t*)z, (const uint16_t*)a, (const uint16_t*)dy, s, sa,
                    (uint16_t*)dw, (uint16_t*)dq, (uint16_t*)dk, (uint16_t*)dv, (uint16_t*)dz, (uint16_t*)da};
    p.chunk_reset = chunk_reset;
    const dim3 grid((unsigned)(B * H));
    if (!chunk_reset) {
        if (ahead) emu::launch(grid, dim3(768), [&] { wkv7v8::bwd_kernel_v8<false, true>(p); });
        else emu::launch(grid, dim3(768), [&] { wkv7v8::bwd_kernel_v8<false>(p); });
    } else if (ahead) emu::launch(grid, dim3(768), [&] { wkv7v8::bwd_kernel_v8<false, true, false, true>(p); });     // schedule 9
    else emu::launch(grid, dim3(768), [&] { wkv7v8::bwd_kernel_v8<false, false, false, true>(p); });                // schedule 8
    return (int)sizeof(wkv7v8::LdsV8);
}
