"""Shared by the tests of the WKV7 training op with a carried state: inputs, the fp64 reference and the limits.

Reference: torch autograd in fp64 through oracle.wkv7_oracle.wkv7_naive(w, q, k, v, z, a, state0) with the loss
sum(y * dy) + sum(state_T * dS_T).  Inputs from oracle.wkv7_oracle.make_inputs; state0 and dS_T seeded normal times 0.1."""
import ctypes

import torch

from oracle.wkv7_oracle import make_inputs, wkv7_naive
from tests.parity import bf16_close, group_bias

# the limits of the existing WKV7 GPU parity tests (tests/test_wkv7_gpu.py), by value
TOL = 1e-3
FLIP_Y, FLIP_G, FLIP_W = 0.01, 0.012, 0.03
# fp32 state gradients (ds0): rel-RMS against the fp64 reference.  Measured for ds_out of the EXISTING sequence-parallel kernel
# (bwd_kernel_v5<.., TPAR>, nseg = 1, parent commit) on these tests' inputs:
#   wave64 emulator, (1, T, 2), T = 16 .. 160, both seeds of a T:   2.28e-6 .. 3.12e-6
#   MI355X, (1,16,1) (2,64,3) (1,384,12) (3,208,5):                 2.77e-6, 2.63e-6, 2.65e-6, 2.55e-6
#   MI355X, the four (b, h) pairs of (16,2624,32) and (8,6400,32):  2.46e-6 .. 2.94e-6
# The limit is twice the SMALLEST of these figures (both kernels sum the same bf16x3 split products in fp32 in another order; a factor of
# two admits reordering noise and nothing systematic), so it holds for every case whichever figure the case itself would have given.
# The new kernel (bwd_kernel_v8<.., STATE>, schedules 8 and 9) measured 2.28e-6 .. 3.12e-6 on the emulator and 2.41e-6 .. 2.94e-6 on the
# MI355X: within 2 % of the v5 figure of the same case.
DS_V5_MEASURED = 2.28e-6
DS_TOL = 2 * DS_V5_MEASURED

NAMES = ("dw", "dq", "dk", "dv", "dz", "da")


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def state_inputs(B, T, H, seed):
    w, q, k, v, z, a, dy = make_inputs(B, T, H, seed=seed)
    g = torch.Generator().manual_seed(1000 + seed)
    s0 = (torch.randn(B, H, 64, 64, generator=g) * 0.1).contiguous()
    dsT = (torch.randn(B, H, 64, 64, generator=g) * 0.1).contiguous()
    return (w, q, k, v, z, a), dy, s0, dsT


def reference(ins, dy, s0=None, dsT=None):
    """fp64 autograd: (y, state_T, [dw, dq, dk, dv, dz, da], ds0); ds0 is None without s0."""
    leaves = [x.double().requires_grad_(True) for x in ins]
    s0l = s0.double().requires_grad_(True) if s0 is not None else None
    y, sT = wkv7_naive(*leaves, state0=s0l)
    loss = (y * dy.double()).sum()
    if dsT is not None:
        loss = loss + (sT * dsT.double()).sum()
    grads = torch.autograd.grad(loss, leaves + ([s0l] if s0l is not None else []))
    return y.detach(), sT.detach(), list(grads[:6]), (grads[6] if s0l is not None else None)


def rel_rms64(x, ref):
    x, ref = x.detach(), ref.detach()
    return float((x.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-300))


def check_grads(got, ref, what, tol=TOL):
    for n, o, r in zip(NAMES, got, ref):
        bf16_close(o, r, f"{what} {n}", tol=tol, max_flip=FLIP_W if n in ("dw", "dz") else FLIP_G)
        group_bias(o, r, f"{what} {n}")
