// csrc/wkv6_step.hip and csrc/decode6_fused.hip -- kernels and C entry points -- compiled for the host lockstep emulator.  TEST INFRASTRUCTURE ONLY.
// (The gated GEMV entry lives in csrc/gemv_decode.hip: emu_gemv_decode.cpp.)
#include <hip/hip_runtime.h>
#include <gfx950_prims.h>
#include "../../visualrwkv_amd/csrc/wkv6_step.hip"
#include "../../visualrwkv_amd/csrc/decode6_fused.hip"
