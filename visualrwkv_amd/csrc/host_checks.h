// The host-side pieces every launcher shares (wkv7_launch.h, ln_fused.hip, tmix_fused.hip and the decode entries: gemv_decode.hip, decode_fused.hip,
// decode6_fused.hip, wkv7_step.hip, wkv6_step.hip): "is one of these pointers NULL", "is one of them off a 16-byte boundary" and "the code of the launches
// just made".
// Host code only, and nothing but hipGetLastError of the runtime: the emulator builds (tests/emu) include it with the translation units that use it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/visualrwkv_hip.h"

namespace hostchk {

template <class... Ptr> inline bool any_null(Ptr... p) { return (... || (p == nullptr)); }
inline bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }      // NULL is not misaligned
template <class... Ptr> inline bool any_misaligned(Ptr... p) { return (... || misaligned(p)); }
// what an entry returns after its launches: VRWKV_OK, or the HIP error of a launch that could not be made
inline int finish_launch() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? VRWKV_OK : (int)e;
}

}  // namespace hostchk
