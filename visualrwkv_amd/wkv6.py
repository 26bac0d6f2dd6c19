"""WKV6 operator surface of the reference (BASELINE config 4), backed by the HIP kernels of csrc/wkv6_chunked.h.

Mirrors VisualRWKV-v6/v6.0/src/model.py:38-88: the extension module's `forward` / `backward` entry points (here
`torch.ops.wkv6.forward / backward`, the schemas of cuda/wkv6_op.cpp:8-13,21-24), the autograd function `WKV_6`
(same asserts, same `ew = -exp(w.float())`, same `gu` reduction over the batch) and `RUN_CUDA_RWKV6`.
Differences a caller cannot see: the forward also writes chunk-start state checkpoints that `WKV_6` keeps for the
backward (the reference re-sweeps the sequence five times instead), and T has no compile-time bound (the reference
sizes a per-thread array with -D_T_=ctx_len).  CPU tensors raise: there is no CPU implementation, as in the reference.

`WKV_6_STATE` / `RUN_CUDA_RWKV6_STATE(B, T, C, H, r, k, v, w, u, s) -> (x, state)` mirror VisualRWKV-v6/v6.xx/src/model.py:35-42 (there a
wrapper over fla's fused_recurrent_rwkv6 with initial_state / output_final_state): the same kernels started from a (B,H,64,64) fp32
[key][value] state, returning the state after the last token, differentiable through both (vrwkv_wkv6_forward_state_bf16 /
vrwkv_wkv6_backward_state_bf16).  All launches go through the state entries; with no state given they run the plain kernels.
"""
from __future__ import annotations

import os

import torch

from . import hip_lib

HEAD_SIZE = 64

_FWD_SCHEMA = ("forward(int B, int T, int C, int H, Tensor r, Tensor k, Tensor v, Tensor w, Tensor u, "
               "Tensor(a!) y) -> ()")
_BWD_SCHEMA = ("backward(int B, int T, int C, int H, Tensor r, Tensor k, Tensor v, Tensor w, Tensor u, Tensor gy, "
               "Tensor(a!) gr, Tensor(b!) gk, Tensor(c!) gv, Tensor(d!) gw, Tensor(e!) gu) -> ()")


def _chk(name, t, shape, dtype):
    if not t.is_cuda:
        raise NotImplementedError("wkv6 has no CPU implementation (neither does the reference: cuda/wkv6_op.cpp "
                                  "binds CUDA kernels only). Move the tensors to an MI355X device.")
    if t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise ValueError(f"wkv6: {name} must be a contiguous {dtype} tensor of shape {tuple(shape)}, "
                         f"got {t.dtype} {tuple(t.shape)} contiguous={t.is_contiguous()}")


def ckpt_tensor(B, T, H, device):
    n = hip_lib.load().vrwkv_wkv6_ckpt_floats(B, T, H)
    return torch.empty(n, dtype=torch.float32, device=device)


# Optional per-launch timing with HIP events on the launch stream (benchmarks/bench_v6.py's roofline leg), as wkv7.EVENT_LOG: when it is a
# list, every launch appends (kind, start_event, end_event, B*T*C).
EVENT_LOG = None


def _launch(name, kind, B, T, C, H, r, *args):
    """One launch of the state entry `name` on r's device (hip_lib.launch), logged in EVENT_LOG as `kind`."""
    with torch.cuda.device(r.device):               # the op surface accepts tensors of any device; hip_lib.launch wants theirs current
        hip_lib.timed(EVENT_LOG, kind, B * T * C, r.device, lambda: hip_lib.launch(name, B, T, C, H, r, *args, device=r.device))


def _chk_state(name, t, B, H):
    if t is not None:
        _chk(name, t, (B, H, HEAD_SIZE, HEAD_SIZE), torch.float32)
    return t


def forward_hip(B, T, C, H, r, k, v, ew, u, y, ckpt=None, state0=None, state_T=None):
    """ew is the f32 log decay the reference's kernels take (`w` of wkv6_op.cpp:8).  state0 / state_T: optional (B,H,64,64) f32
    [key][value] states before token 0 / after token T-1 (None: zeros / not wanted; with both None the state entry IS the plain one)."""
    bf = torch.bfloat16
    for n, t in (("r", r), ("k", k), ("v", v), ("y", y)):
        _chk(n, t, (B, T, C), bf)
    _chk("w", ew, (B, T, C), torch.float32)
    if u.numel() != C:
        raise ValueError(f"wkv6: u must have {C} elements")
    _chk("u", u, u.shape, bf)
    s0, sT = _chk_state("state0", state0, B, H), _chk_state("state_T", state_T, B, H)
    _launch("vrwkv_wkv6_forward_state_bf16", "fwd", B, T, C, H, r, k, v, ew, u, s0, y, sT, ckpt)


def backward_hip(B, T, C, H, r, k, v, ew, u, gy, gr, gk, gv, gw, gu, ckpt=None, state0=None, d_state_T=None, d_state0=None):
    """d_state_T / d_state0: optional (B,H,64,64) f32 gradients of the state after the last / before the first token (None: zeros / not
    wanted).  state0 is read only when the checkpoints are regenerated here: a saved `ckpt` already starts from it."""
    bf = torch.bfloat16
    for n, t in (("r", r), ("k", k), ("v", v), ("gy", gy), ("gr", gr), ("gk", gk), ("gv", gv), ("gw", gw)):
        _chk(n, t, (B, T, C), bf)
    _chk("w", ew, (B, T, C), torch.float32)
    _chk("u", u, u.shape, bf)
    _chk("gu", gu, (B, C), bf)
    if ckpt is None:            # reference calling convention: no saved state -> regenerate the checkpoints
        ckpt = ckpt_tensor(B, T, H, r.device)
        forward_hip(B, T, C, H, r, k, v, ew, u, torch.empty_like(r), ckpt, state0)
    dT, d0 = _chk_state("d_state_T", d_state_T, B, H), _chk_state("d_state0", d_state0, B, H)
    _launch("vrwkv_wkv6_backward_state_bf16", "bwd", B, T, C, H, r, k, v, ew, u, gy, ckpt, dT, gr, gk, gv, gw, gu, d0)


def _apply_variant_env():
    """VRWKV_WKV6_BWD_VARIANT: same-box A/B of the backward kernel generations (benchmarks only)."""
    v = os.environ.get("VRWKV_WKV6_BWD_VARIANT")
    if v is not None:
        hip_lib.check(hip_lib.load().vrwkv_wkv6_set_backward_variant(int(v)), "vrwkv_wkv6_set_backward_variant")


def _register():
    lib = torch.library.Library("wkv6", "DEF")
    lib.define(_FWD_SCHEMA)
    lib.define(_BWD_SCHEMA)
    lib.impl("forward", lambda B, T, C, H, r, k, v, w, u, y: forward_hip(B, T, C, H, r, k, v, w, u, y), "CUDA")
    lib.impl("backward", lambda B, T, C, H, r, k, v, w, u, gy, gr, gk, gv, gw, gu:
             backward_hip(B, T, C, H, r, k, v, w, u, gy, gr, gk, gv, gw, gu), "CUDA")

    def no_cpu(*a):
        raise NotImplementedError("wkv6 has no CPU implementation; move the tensors to an MI355X device")
    lib.impl("forward", no_cpu, "CPU")
    lib.impl("backward", no_cpu, "CPU")
    return lib


_LIB = _register()
_apply_variant_env()


class WKV_6(torch.autograd.Function):
    """VisualRWKV-v6/v6.0/src/model.py:43-85."""

    @staticmethod
    def forward(ctx, B, T, C, H, r, k, v, w, u):
        with torch.no_grad():
            assert all(x.dtype == torch.bfloat16 for x in (r, k, v, w, u))
            assert HEAD_SIZE == C // H
            assert all(x.is_contiguous() for x in (r, k, v, w, u))
            ctx.B, ctx.T, ctx.C, ctx.H = B, T, C, H
            ew = (-torch.exp(w.float())).contiguous()
            y = torch.empty((B, T, C), device=r.device, dtype=torch.bfloat16)
            ckpt = ckpt_tensor(B, T, H, r.device) if any(ctx.needs_input_grad) else None
            forward_hip(B, T, C, H, r, k, v, ew, u, y, ckpt)
            ctx.save_for_backward(r, k, v, ew, u, ckpt)
            return y

    @staticmethod
    def backward(ctx, gy):
        with torch.no_grad():
            assert gy.dtype == torch.bfloat16
            B, T, C, H = ctx.B, ctx.T, ctx.C, ctx.H
            gy = gy.contiguous()
            r, k, v, ew, u, ckpt = ctx.saved_tensors
            gr, gk, gv, gw = (torch.empty((B, T, C), device=gy.device, dtype=torch.bfloat16) for _ in range(4))
            gu = torch.empty((B, C), device=gy.device, dtype=torch.bfloat16)
            backward_hip(B, T, C, H, r, k, v, ew, u, gy, gr, gk, gv, gw, gu, ckpt)
            gu = torch.sum(gu, 0).view(H, C // H)
            return (None, None, None, None, gr, gk, gv, gw, gu)


def RUN_CUDA_RWKV6(B, T, C, H, r, k, v, w, u):
    return WKV_6.apply(B, T, C, H, r, k, v, w, u)


class WKV_6_STATE(torch.autograd.Function):
    """WKV_6 with a carried state: what RUN_CUDA_RWKV6_STATE of VisualRWKV-v6/v6.xx/src/model.py:35-42 computes through fla's
    fused_recurrent_rwkv6(initial_state=, output_final_state=True), forward and backward.  `s`: (B,H,64,64) f32 [key][value] or None (zeros).
    Returns (y bf16, state f32 or None with want_state=False).  dL/ds is produced only when `s` needs it; dL/d(state) enters only when the returned state got a gradient."""

    @staticmethod
    def forward(ctx, B, T, C, H, r, k, v, w, u, s, want_state=True):
        with torch.no_grad():
            assert all(x.dtype == torch.bfloat16 for x in (r, k, v, w, u))
            assert HEAD_SIZE == C // H
            assert all(x.is_contiguous() for x in (r, k, v, w, u))
            ctx.B, ctx.T, ctx.C, ctx.H = B, T, C, H
            ctx.set_materialize_grads(False)
            ew = (-torch.exp(w.float())).contiguous()
            y = torch.empty((B, T, C), device=r.device, dtype=torch.bfloat16)
            state = torch.empty((B, H, HEAD_SIZE, HEAD_SIZE), device=r.device, dtype=torch.float32) if want_state else None
            ckpt = ckpt_tensor(B, T, H, r.device) if any(ctx.needs_input_grad) else None
            forward_hip(B, T, C, H, r, k, v, ew, u, y, ckpt, s.contiguous() if s is not None else None, state)
            ctx.save_for_backward(r, k, v, ew, u, ckpt)          # the checkpoint of chunk 0 holds s
            return y, state

    @staticmethod
    def backward(ctx, gy, gstate):
        with torch.no_grad():
            B, T, C, H = ctx.B, ctx.T, ctx.C, ctx.H
            r, k, v, ew, u, ckpt = ctx.saved_tensors
            if gy is None:
                gy = torch.zeros((B, T, C), device=r.device, dtype=torch.bfloat16)
            assert gy.dtype == torch.bfloat16
            gy = gy.contiguous()
            gr, gk, gv, gw = (torch.empty((B, T, C), device=gy.device, dtype=torch.bfloat16) for _ in range(4))
            gu = torch.empty((B, C), device=gy.device, dtype=torch.bfloat16)
            gs = torch.empty((B, H, HEAD_SIZE, HEAD_SIZE), device=gy.device, dtype=torch.float32) if ctx.needs_input_grad[9] else None
            backward_hip(B, T, C, H, r, k, v, ew, u, gy, gr, gk, gv, gw, gu, ckpt,
                         d_state_T=gstate.float().contiguous() if gstate is not None else None, d_state0=gs)
            gu = gu.float().sum(0).view(H, C // H).to(u.dtype)         # per-sample bf16 rows, summed in fp32
            return (None, None, None, None, gr, gk, gv, gw, gu, gs, None)


def RUN_CUDA_RWKV6_STATE(B, T, C, H, r, k, v, w, u, s, want_state=True):
    """-> (x, state): VisualRWKV-v6/v6.xx/src/model.py:35-42.  want_state=False (not in the reference): the final state is not written and
    None is returned for it."""
    return WKV_6_STATE.apply(B, T, C, H, r, k, v, w, u, s, want_state)
