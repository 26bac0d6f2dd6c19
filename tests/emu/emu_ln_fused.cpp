// csrc/ln_fused.hip -- the C entry points with their launch logic (grid caps, ws split, LB dispatch, NULL switches) -- compiled for the host
// lockstep emulator: the same vrwkv_add_ln_* / vrwkv_ln_mix_* / vrwkv_ln_scatter_* / vrwkv_ln_gather_* symbols as the product library, computed
// on the CPU with the product's own cap values.  TEST INFRASTRUCTURE ONLY.
#include <hip/hip_runtime.h>
#include <gfx950_prims.h>
namespace {                 // emu_ln.cpp holds the external definitions of this header's non-template kernels
#include <ln_kernels.h>
}
#include "../../visualrwkv_amd/csrc/ln_fused.hip"
