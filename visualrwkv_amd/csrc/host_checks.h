// The host-side pieces of every translation unit with a stream entry: "is one of these pointers NULL", "is one of them off a 16-byte boundary", "the
// code of the launches just made", the dynamic-LDS launch and the capped grid of the grid-stride streaming kernels.  (patch_embed.hip alone spells its
// alignment out: its pixels, weight and rows are held to 4, 16 and 8 bytes.)
// Host code only, and of the runtime nothing but hipGetLastError, hipFuncSetAttribute and the launch: the emulator builds (tests/emu) include it with
// the translation units that use it.
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
// dynamic-LDS launch of a kernel taking one argument block
template <class Args>
inline int launch_lds(void (*kern)(Args), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const Args& p) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kern, grid, block, lds_bytes, st, p);
    return finish_launch();
}
// workgroups of 256 threads for nvec 16-byte pieces: <= 8 per CU, the kernel grid-strides the rest
inline int grid_for(long nvec) {
    long b = (nvec + 255) / 256;
    return (int)(b < 1 ? 1 : b > 2048 ? 2048 : b);
}

}  // namespace hostchk
