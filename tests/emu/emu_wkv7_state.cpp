// The STATE instantiations of wkv7_bwd_v8.h (the training backward with a carried state: dL/dS in and out, S0 of chunk 0 from the state the
// forward started from) under the host lockstep emulator.  TEST INFRASTRUCTURE ONLY -- the C entry on top of them
// (vrwkv_wkv7_backward_state_bf16) comes in through emu_wkv7_capi.cpp.
#include <gfx950_prims.h>   // resolves to tests/emu/gfx950_prims.h (-I order)
#include <wkv7_kernels.h>
#include <wkv7_chunked.h>
#include <wkv7_bwd_v6.h>
#include <wkv7_bwd_v8.h>

extern "C" int emu_wkv7_backward_state_v8(int B, int T, int H, const void* w, const void* q, const void* k, const void* v,
                                          const void* z, const void* a, const void* dy, const float* s, const float* sa,
                                          const float* s0, const float* ds_in, float* ds_out,
                                          void* dw, void* dq, void* dk, void* dv, void* dz, void* da, int ahead) {
    wkv7::BwdArgs p{T, H, (const uint16_t*)w, (const uint16_t*)q, (const uint16_t*)k, (const uint16_t*)v,
                    (const uint16_t*)z, (const uint16_t*)a, (const uint16_t*)dy, s, sa,
                    (uint16_t*)dw, (uint16_t*)dq, (uint16_t*)dk, (uint16_t*)dv, (uint16_t*)dz, (uint16_t*)da};
    p.ds_in = ds_in; p.ds_out = ds_out; p.s0 = s0; p.want_grads = 1;
    const dim3 grid((unsigned)(B * H));
    if (ahead) emu::launch(grid, dim3(768), [&] { wkv7v8::bwd_kernel_v8<false, true, true>(p); });     // schedule 9: score pieces a step ahead
    else emu::launch(grid, dim3(768), [&] { wkv7v8::bwd_kernel_v8<false, false, true>(p); });         // schedule 8
    return (int)sizeof(wkv7v8::LdsV8);
}
