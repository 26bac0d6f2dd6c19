// csrc/wkv6_capi.hip -- the WKV6 launchers (plain and state entries, argument checks, kernel generation and STATE instantiation selection,
// batch slices) and the kernels behind them -- compiled whole for the host lockstep emulator.  TEST INFRASTRUCTURE ONLY.
#include <hip/hip_runtime.h>
#include <gfx950_prims.h>
#include "../../visualrwkv_amd/csrc/wkv6_capi.hip"
