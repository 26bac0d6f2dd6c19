// csrc/sample_head.hip -- kernel and C entry point -- compiled for the host lockstep emulator.  TEST INFRASTRUCTURE ONLY.
#include <hip/hip_runtime.h>
#include <gfx950_prims.h>
#include "../../visualrwkv_amd/csrc/sample_head.hip"
