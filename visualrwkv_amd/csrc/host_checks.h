// The two host-side pieces every launcher shares (wkv7_launch.h, ln_fused.hip, tmix_fused.hip): "is one of these pointers NULL" and "the code of the launches just made".
// Host code only, and nothing but hipGetLastError of the runtime: the emulator builds (tests/emu) include it with the translation units that use it.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/visualrwkv_hip.h"

namespace hostchk {

template <class... Ptr> inline bool any_null(Ptr... p) { return (... || (p == nullptr)); }
// what an entry returns after its launches: VRWKV_OK, or the HIP error of a launch that could not be made
inline int finish_launch() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? VRWKV_OK : (int)e;
}

}  // namespace hostchk
