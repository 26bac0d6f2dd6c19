"""Fused HIP implementations of the element-wise glue of RWKV_Tmix_x070 / RWKV_CMix_x070.

Enabled per model with `args.fused = True` (rwkv7.py dispatches here for CUDA tensors).  Each autograd
Function below is one forward kernel and one backward kernel of csrc/tmix_fused.hip; the dense projections
stay hipBLASLt GEMMs (plain `F.linear` / `@`).  There is no fallback: tensors must be bf16, contiguous, on an
MI355X -- anything else raises.
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from . import gemm_tuning, hip_lib
from .wkv7 import RUN_CUDA_RWKV7g, RUN_CUDA_RWKV7g_packed, RUN_CUDA_RWKV7g_state


def _chk(*ts):
    for t in ts:
        if t is None:
            continue
        if not (t.is_cuda and t.dtype == torch.bfloat16 and t.is_contiguous()):
            raise ValueError("fused RWKV-7 kernels need contiguous bf16 tensors on the GPU "
                             f"(got {t.dtype}, cuda={t.is_cuda}, contiguous={t.is_contiguous()})")


def _ws(ntok, C, nvec, device):
    n = hip_lib.load().vrwkv_param_grad_ws_floats(ntok, C, nvec)
    return torch.empty(n, dtype=torch.float32, device=device)


def _glue(name, *args, like):
    """One launch of the library entry `name` on PyTorch's current stream of like's device -- read now, so under `torch.cuda.stream(side)` it is the
    side stream: hip_lib.launch says how `args` reach the entry."""
    hip_lib.launch(name, *args, device=like.device)


def _grad_rows(ntok, C, nvec, device):
    """What a glue backward entry writes its parameter gradients through: (the nvec fp32 rows of C, the workspace of its partial rows)."""
    return torch.empty(nvec, C, dtype=torch.float32, device=device), _ws(ntok, C, nvec, device)


def _rows_as(pg, dtype, shapes):
    """The fp32 gradient rows in the parameters' dtype, row i in the shape shapes[i] (None: there is no such parameter)."""
    pg = pg.to(dtype)
    return [pg[i].view(s) if s is not None else None for i, s in enumerate(shapes)]


def wgrad_skinny_supported(x2d, dy2d):
    K, N = x2d.shape[1], dy2d.shape[1]
    nw, d = max(K, N), min(K, N)
    return (x2d.is_cuda and x2d.dtype == torch.bfloat16 and dy2d.dtype == torch.bfloat16 and nw % 128 == 0
            and d in (32, 64, 96, 128, 160, 256) and nw > d)


def wgrad_skinny(x2d, dy2d):
    """x2d^T dy2d for (M,K), (M,N) with one of K, N a LoRA rank: csrc/lora_wgrad.h (the library's kernels for this
    shape -- reduction over ~42 k tokens, one operand 64-256 columns wide -- run 3-4x above the cost of reading the
    wide operand once).  Returns (K,N) bf16."""
    x2d, dy2d = x2d.contiguous(), dy2d.contiguous()
    M, K = x2d.shape
    N = dy2d.shape[1]
    wide, narrow, transposed = (x2d, dy2d, 0) if K >= N else (dy2d, x2d, 1)
    nws = hip_lib.load().vrwkv_wgrad_skinny_ws_floats(M, wide.shape[1], narrow.shape[1])
    if nws < 0:
        raise ValueError(f"wgrad_skinny: unsupported shape ({M},{K}) x ({M},{N})")
    ws = torch.empty(nws, dtype=torch.float32, device=x2d.device)
    out = torch.empty(K, N, dtype=torch.bfloat16, device=x2d.device)
    _glue("vrwkv_wgrad_skinny_bf16", M, wide.shape[1], narrow.shape[1], wide, narrow, out, transposed, ws, like=x2d)
    return out


LORA_UP = os.environ.get("VRWKV_LORA_UP", "1") != "0"            # A/B switch: 0 = the library's GEMM for the write-wide products a (M, r) . w -> (M, C)
SKINNY_UP_RANKS = (32, 64, 96, 128, 160, 256)
# (rank, w_is_CxR) pairs that run on csrc/skinny_up.h: the ones that beat the library's best kernel for the shape by more than 10 % at M = 41 984,
# C = 2048 (benchmarks/lora_gemm_micro.py); a pair that does not stays on the library.  profiles/skinny_up_micro.jsonl: all twelve do, by 32 %
# (r = 256, w as C x r) to 107 %, with bit-equal results.
SKINNY_UP_CASES = frozenset((r, l) for r in SKINNY_UP_RANKS for l in (0, 1))


def skinny_up_supported(a2d, w, w_is_CxR):
    """a2d (M, R) . w (R, C), or a2d . w^T for w (C, R) with w_is_CxR: whether csrc/skinny_up.h takes it."""
    if not (LORA_UP and a2d.dim() == 2 and w.dim() == 2 and a2d.is_cuda and w.is_cuda and a2d.dtype == torch.bfloat16 and w.dtype == torch.bfloat16
            and a2d.is_contiguous() and w.is_contiguous() and a2d.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0):
        return False
    R = a2d.shape[1]
    C, Rw = (w.shape[0], w.shape[1]) if w_is_CxR else (w.shape[1], w.shape[0])
    return Rw == R and (R, int(bool(w_is_CxR))) in SKINNY_UP_CASES and C % 128 == 0 and C > R and a2d.shape[0] >= 1


def skinny_up(a2d, w, w_is_CxR):
    """The write-wide product of a LoRA pair on csrc/skinny_up.h.  Returns (M, C) bf16."""
    M, R = a2d.shape
    C = w.shape[0] if w_is_CxR else w.shape[1]
    out = torch.empty(M, C, dtype=torch.bfloat16, device=a2d.device)
    _glue("vrwkv_skinny_up_bf16", M, R, C, a2d, w, int(bool(w_is_CxR)), out, like=a2d)
    return out


def _lora_product(a, w, w_is_CxR):
    """a @ w (w_is_CxR = 0) or a @ w.t(): the own kernel for the write-wide shapes it takes, the library for everything else."""
    if LORA_UP and a.is_cuda and a.is_contiguous():
        a2d = a.view(-1, a.shape[-1])
        if skinny_up_supported(a2d, w, w_is_CxR):
            return skinny_up(a2d, w, w_is_CxR).view(*a.shape[:-1], -1)
    return a @ w.t() if w_is_CxR else a @ w


class _LoraMM(torch.autograd.Function):
    """x @ w for a LoRA factor w (C x rank or rank x C): csrc/skinny_up.h for the write-wide output (w rank x C) and the write-wide
    input gradient (w C x rank), library GEMMs for the read-wide ones, the skinny weight-gradient kernel for dw
    (src/model.py:176,181-183 -- plain `@` in the reference)."""

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        return _lora_product(x, w, 0)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dx = _lora_product(dy, w, 1) if ctx.needs_input_grad[0] else None
        dw = None
        if ctx.needs_input_grad[1]:
            x2d, dy2d = x.reshape(-1, x.shape[-1]), dy.reshape(-1, dy.shape[-1])
            dw = wgrad_skinny(x2d, dy2d) if wgrad_skinny_supported(x2d, dy2d) else x2d.t() @ dy2d
        return dx, dw


lora_mm = _LoraMM.apply
LORA_WGRAD = os.environ.get("VRWKV_LORA_WGRAD", "1") != "0"      # A/B switch for benchmarks: 0 = autograd's torch.mm
GRAD_ALIAS = os.environ.get("VRWKV_GRAD_ALIAS", "1") != "0"      # A/B switch: 0 = autograd sums the gradients of x_v, k2, v2
DGRAD_TN = os.environ.get("VRWKV_DGRAD_TN", "1") != "0"          # A/B switch: 0 = autograd's dy.mm(W) for the input gradient of Linear
VF_CHAIN = os.environ.get("VRWKV_VF_CHAIN", "1") != "0"          # A/B switch: 0 = every layer returns its own v_first gradient term, autograd adds them
FLAT_WGRAD = os.environ.get("VRWKV_FLAT_WGRAD", "1") != "0"      # A/B switch: 0 = weight gradients as fresh tensors, copied into the ZeRO-1 buffer


# dgrad (library GEMM) and wgrad (csrc/wgrad_big.h) of one Linear on two HIP streams, joined before the node returns: both are whole-chip kernels whose LAST
# round of workgroups is part-filled (C x C at 41 984 rows: 5.125 rounds of 256 x 256 tiles cost 6, profiles/r6h_gemm_tail_probe.jsonl), and a kernel of another
# stream takes the idle CUs.  The streams never leave the autograd node, so what autograd and the ZeRO-1 hooks see is unchanged.  0 = one after the other.
# (The same for the skinny LoRA products measured +0.7 % -- two 50 us memory-bound kernels gain less than the two stream joins cost -- and is not done.)
# SAFETY: the side stream carries only this package's own kernels (wgrad_big, relu^2), never a second LIBRARY GEMM: hipBLASLt's default pick for large
# shapes is a stream-K kernel whose workgroups spin on each other, and two of those on two streams deadlock the GPU (gemm_tuning's docstring).  Where both
# sides would be library GEMMs (the r/k/v forward, a weight gradient the library computes) the streams are used only for shapes listed as checked in the
# loaded tuning file's sidecar (gemm_tuning.concurrent_ok); everything else runs one after the other.
OVERLAP_WGRAD = os.environ.get("VRWKV_OVERLAP_WGRAD", "1") != "0"
_SIDE_STREAMS = {}


def _side_stream(dev, i=0):
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), i)
    st = _SIDE_STREAMS.get(key)
    if st is None:
        st = _SIDE_STREAMS[key] = torch.cuda.Stream(device=dev)
    return st


BIG_WGRAD = os.environ.get("VRWKV_BIG_WGRAD", "1") != "0"        # A/B switch: 0 = the library's "N,T" kernel for dW = dy^T x of the Linear layers


def wgrad_big_supported(dy2d, x2d):
    return (BIG_WGRAD and dy2d.is_cuda and dy2d.dtype == torch.bfloat16 and x2d.dtype == torch.bfloat16 and dy2d.is_contiguous()
            and x2d.is_contiguous() and dy2d.shape[0] > 0 and dy2d.shape[0] % 32 == 0 and dy2d.shape[1] % 256 == 0 and x2d.shape[1] % 256 == 0
            and max(dy2d.shape[1], x2d.shape[1]) <= 16384)      # the head (65 536 x 2048): the library is 4 % faster (profiles/r4_wgrad_big_micro.jsonl)


def wgrad_big(dy2d, x2d, out=None):
    """dy2d^T x2d for (M,N), (M,K) -> (N,K) bf16 (the weight gradient of nn.Linear, src/model.py:150-153,214-215,281) with
    csrc/wgrad_big.h instead of the library's N,T-class kernel; `out`: a contiguous (N,K) bf16 view to write into."""
    M, N = dy2d.shape
    K = x2d.shape[1]
    nws = hip_lib.load().vrwkv_wgrad_big_ws_floats(M, N, K)
    if nws < 0:
        raise ValueError(f"wgrad_big: unsupported shape ({M},{N}) x ({M},{K})")
    ws = torch.empty(nws, dtype=torch.float32, device=dy2d.device) if nws else None
    if out is None:
        out = torch.empty(N, K, dtype=torch.bfloat16, device=dy2d.device)
    _glue("vrwkv_wgrad_big_bf16", M, N, K, dy2d, x2d, out, ws, like=dy2d)
    return out


def _wgrad_beside_dgrad(wp, dy2, x2):
    """May dW = dy2^T x2 run on the side stream while the library computes the input gradient?  Yes when it is csrc/wgrad_big.h (the same conditions as
    in _weight_grad), or when this shape's pair of library kernels is listed as checked."""
    if not (OVERLAP_WGRAD and dy2.is_cuda):
        return False
    flat = (FLAT_WGRAD and wp is not None and wp.grad is None and getattr(wp, "_vrwkv_flat_armed", False)
            and not getattr(wp, "_vrwkv_wgrad_pending", False) and wp._vrwkv_flat_grad[0].dtype == dy2.dtype)
    if wgrad_big_supported(dy2, x2) and (not flat or wp._vrwkv_flat_grad[1] % 8 == 0):
        return True
    return gemm_tuning.concurrent_ok(f"dgrad+wgrad {dy2.shape[0]}x{dy2.shape[1]}x{x2.shape[1]}")


def _weight_grad(wp, dy2, x2):
    """dW = dy2^T x2 (N,K) for a Linear weight; `wp` = the Parameter when a ZeRO-1 engine (dp.Zero1Engine) armed by its zero_grad() owns
    its gradient slot, else None.  First gradient of an armed weight in the step: the GEMM writes into the weight's slot of the flat
    gradient buffer; autograd adopts the returned view as `.grad` and the engine finds it in place.  `pending` until the engine's hook has
    seen it: a second use of the same weight in one graph (two forward passes under one backward) must not write the slot again while
    autograd still holds the first gradient there."""
    if (FLAT_WGRAD and wp is not None and wp.grad is None and getattr(wp, "_vrwkv_flat_armed", False)
            and not getattr(wp, "_vrwkv_wgrad_pending", False) and wp._vrwkv_flat_grad[0].dtype == dy2.dtype):
        flat, o = wp._vrwkv_flat_grad
        dw = flat[o:o + wp.numel()].view(wp.shape)
        if wgrad_big_supported(dy2, x2) and o % 8 == 0:
            wgrad_big(dy2, x2, out=dw)
        else:
            torch.mm(dy2.t(), x2, out=dw)
        wp._vrwkv_wgrad_pending = True
        return dw
    if wgrad_big_supported(dy2, x2):
        return wgrad_big(dy2, x2)
    return dy2.t().mm(x2)


class _LinearTN(torch.autograd.Function):
    """F.linear(x, W) whose input gradient is issued in the layout of the forward GEMMs.  Autograd computes dx = dy.mm(W)
    with W (N_out, K_in) row-major: the contraction index is the strided one of W (hipBLASLt "N,N"), 8-15 % slower on
    MI355X than the "T,N" kernels the forward gets (both operands contraction-contiguous; measured 908 vs 1229 TFLOP/s at
    41 984 x 2048 x 2048, benchmarks/dgrad_layout_micro.py).  Here dx = F.linear(dy, W^T) on a transposed copy of the
    weight (31-77 us per weight, included in the measurement): the same T,N kernels as the forward.  dW: _weight_grad."""

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        ctx.wparam = w if hasattr(w, "_vrwkv_flat_grad") else None      # the Parameter itself (saved_tensors hands back a plain tensor)
        return F.linear(x, w)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dx = dw = None
        if ctx.needs_input_grad[0] and ctx.needs_input_grad[1] and dy.is_cuda:
            dy = dy.contiguous()
        if (ctx.needs_input_grad[0] and ctx.needs_input_grad[1]
                and _wgrad_beside_dgrad(ctx.wparam, dy.reshape(-1, dy.shape[-1]), x.reshape(-1, x.shape[-1]))):
            cur, side = torch.cuda.current_stream(dy.device), _side_stream(dy.device)
            side.wait_stream(cur)                                    # dy and x are ready
            with torch.cuda.stream(side):
                dw = _weight_grad(ctx.wparam, dy.reshape(-1, dy.shape[-1]), x.reshape(-1, x.shape[-1]))
            dx = F.linear(dy, transpose2d(w))
            cur.wait_stream(side)                                    # joined: nothing of the side stream outlives this node
            dw.record_stream(cur)
            return dx, dw
        if ctx.needs_input_grad[0]:
            dx = F.linear(dy, transpose2d(w))
        if ctx.needs_input_grad[1]:
            dw = _weight_grad(ctx.wparam, dy.reshape(-1, dy.shape[-1]), x.reshape(-1, x.shape[-1]))
        return dx, dw


class _Linear3TN(torch.autograd.Function):
    """Three independent bias-free Linear layers on three inputs -- receptance / key / value of the time-mix (src/model.py:175-178) -- as ONE autograd node
    whose GEMMs run on three HIP streams (forward) and whose input-gradient and weight-gradient GEMMs run on two (backward), joined before the node
    returns (see OVERLAP_WGRAD): each of these C x C GEMMs alone leaves 7/8 of its last round of tiles idle."""

    @staticmethod
    def forward(ctx, x0, x1, x2, w0, w1, w2):
        ctx.save_for_backward(x0, x1, x2, w0, w1, w2)
        ctx.wparams = [w if hasattr(w, "_vrwkv_flat_grad") else None for w in (w0, w1, w2)]
        M = x0.numel() // x0.shape[-1]
        if not gemm_tuning.concurrent_ok(f"3x tn_{w0.shape[0]}_{M}_{w0.shape[1]}"):       # three library GEMMs at once: checked shapes only (see OVERLAP_WGRAD)
            return F.linear(x0, w0), F.linear(x1, w1), F.linear(x2, w2)
        cur = torch.cuda.current_stream(x0.device)
        sides = [_side_stream(x0.device, 0), _side_stream(x0.device, 1)]
        outs = [None, None, None]
        for st, i, x, w in ((sides[0], 1, x1, w1), (sides[1], 2, x2, w2)):
            st.wait_stream(cur)
            with torch.cuda.stream(st):
                outs[i] = F.linear(x, w)
        outs[0] = F.linear(x0, w0)
        for st, i in ((sides[0], 1), (sides[1], 2)):
            cur.wait_stream(st)
            outs[i].record_stream(cur)
        return tuple(outs)

    @staticmethod
    def backward(ctx, d0, d1, d2):
        x0, x1, x2, w0, w1, w2 = ctx.saved_tensors
        dys = [d.contiguous() for d in (d0, d1, d2)]
        jobs = [(wp, dy.reshape(-1, dy.shape[-1]), x.reshape(-1, x.shape[-1])) for wp, dy, x in zip(ctx.wparams, dys, (x0, x1, x2))]
        beside = all(_wgrad_beside_dgrad(*j) for j in jobs)
        cur = torch.cuda.current_stream(x0.device)
        side = _side_stream(x0.device) if beside else cur
        if beside:
            side.wait_stream(cur)
        with torch.cuda.stream(side):
            dws = [_weight_grad(*j) for j in jobs]
        dxs = [F.linear(dy, transpose2d(w)) for dy, w in zip(dys, (w0, w1, w2))]
        if beside:
            cur.wait_stream(side)
            for dw in dws:
                dw.record_stream(cur)
        return (*dxs, *dws)


def linear3(modules, xs):
    """(m(x) for m, x in zip(modules, xs)) for three bias-free nn.Linear of equal shape; one node with internal stream concurrency in training on the GPU."""
    if (OVERLAP_WGRAD and DGRAD_TN and all(m.bias is None for m in modules) and all(x.is_cuda and x.requires_grad for x in xs) and torch.is_grad_enabled()
            and all(m.weight.requires_grad for m in modules)):
        return _Linear3TN.apply(*xs, *[m.weight for m in modules])
    return tuple(linear(m, x) for m, x in zip(modules, xs))


def transpose2d(w):
    """w.t().contiguous() for a 2-D bf16 matrix: tiled HIP kernel when both sides are multiples of 64 (3-4x torch's copy)."""
    if w.is_cuda and w.dtype == torch.bfloat16 and w.dim() == 2 and w.is_contiguous() and w.shape[0] % 64 == 0 and w.shape[1] % 64 == 0:
        out = torch.empty(w.shape[1], w.shape[0], dtype=w.dtype, device=w.device)
        _glue("vrwkv_transpose_bf16", w.shape[0], w.shape[1], w, out, like=w)
        return out
    return w.t().contiguous()


def linear(module, x):
    """module(x) for a bias-free nn.Linear; in training on the GPU through _LinearTN."""
    if DGRAD_TN and module.bias is None and x.is_cuda and torch.is_grad_enabled() and x.requires_grad:
        return _LinearTN.apply(x, module.weight)
    return module(x)


class _Mix(torch.autograd.Function):
    """token-shift + M lerps:  out_m = x + (shift(x) - x) * mu_m."""

    @staticmethod
    def forward(ctx, x, *mus):
        return _Mix._forward(ctx, False, x, *mus)

    @staticmethod
    def _forward(ctx, dup3, x, *mus):
        B, T, C = x.shape
        x = x.contiguous()
        mus_c = [m.reshape(C).contiguous() for m in mus]
        _chk(x, *mus_c)
        outs = [torch.empty_like(x) for _ in mus]
        _glue("vrwkv_mix_fwd_bf16", B * T, T, C, len(mus), x, mus_c, outs, like=x)
        ctx.save_for_backward(x, *mus_c)
        ctx.mu_shapes = [m.shape for m in mus]
        if dup3:                 # a 7th output aliasing output 3 (x_v) for its second consumer
            outs.append(outs[3].view_as(outs[3]))
        return tuple(outs)

    @staticmethod
    def backward(ctx, *douts):
        x, *mus_c = ctx.saved_tensors
        B, T, C = x.shape
        douts = [d.contiguous() for d in douts]
        _chk(*douts)
        M = len(mus_c)
        second = douts[M] if len(douts) > M else None          # gradient of the alias of output 3
        dx = torch.empty_like(x)
        dmu, ws = _grad_rows(B * T, C, M, x.device)
        _glue("vrwkv_mix_bwd2_bf16", B * T, T, C, M, x, mus_c, douts[:M], second, dx, dmu, ws, like=x)
        return (dx, *_rows_as(dmu, x.dtype, ctx.mu_shapes))


class _MixDup3(_Mix):
    """`_Mix` for the time-mix of layers > 0: x_v is returned twice (the second an alias) so that the gradients of its two
    consumers reach mix_bwd as separate inputs and are summed there, not by an element-wise kernel of autograd."""

    @staticmethod
    def forward(ctx, x, *mus):
        return _Mix._forward(ctx, True, x, *mus)


class _Decay(torch.autograd.Function):
    """w = -softplus(-(w0 + h)) - 0.5"""

    @staticmethod
    def forward(ctx, h, w0):
        h = h.contiguous()
        C = h.shape[-1]
        w0c = w0.reshape(C).contiguous()
        _chk(h, w0c)
        w = torch.empty_like(h)
        _glue("vrwkv_decay_fwd_bf16", h.numel() // C, C, h, w0c, w, like=h)
        ctx.save_for_backward(h, w0c)
        ctx.w0_shape = w0.shape
        return w

    @staticmethod
    def backward(ctx, dw):
        h, w0c = ctx.saved_tensors
        C = h.shape[-1]
        dw = dw.contiguous()
        _chk(dw)
        dh = torch.empty_like(h)
        dw0, ws = _grad_rows(h.numel() // C, C, 1, h.device)
        _glue("vrwkv_decay_bwd_bf16", h.numel() // C, C, h, w0c, dw, dh, dw0, ws, like=h)
        return dh, *_rows_as(dw0, h.dtype, [ctx.w0_shape])


class _Kva(torch.autograd.Function):
    """(k, v, v_first, vl, al; k_k, k_a, a0, v0) -> (k2, v2, z, b); v/v_first/vl/v0 are None for layer 0.
    dup=True appends aliases of k2 (and v2) for a second consumer: their gradients reach the backward kernel as
    separate inputs and are summed there (autograd would run one 3 x 172 MB element-wise add per tensor and layer).
    chain=True (layers > 0) appends an alias of v_first, which the NEXT layer uses as its v_first: the gradient of v_first then
    travels down the layers as one running sum that each kva backward adds its term to, instead of 23 terms for autograd to add."""

    @staticmethod
    def forward(ctx, k, v, v_first, vl, al, k_k, k_a, a0, v0, *flags):
        dup = bool(flags[0]) if len(flags) > 0 else False
        has = v is not None
        chain = (bool(flags[1]) if len(flags) > 1 else False) and has
        ctx.nflags = len(flags)
        ctx.set_materialize_grads(False)         # the last layer's alias of v_first has no consumer: its gradient arrives as None
        k, al = k.contiguous(), al.contiguous()
        C = k.shape[-1]
        ntok = k.numel() // C
        if has:
            v, v_first, vl = v.contiguous(), v_first.contiguous(), vl.contiguous()
        pk, pa, p0 = k_k.reshape(C).contiguous(), k_a.reshape(C).contiguous(), a0.reshape(C).contiguous()
        pv = v0.reshape(C).contiguous() if has else None
        _chk(k, al, v, v_first, vl, pk, pa, p0, pv)
        k2, z, b = torch.empty_like(k), torch.empty_like(k), torch.empty_like(k)
        v2 = torch.empty_like(k) if has else None
        _glue("vrwkv_kva_fwd_bf16", ntok, C, int(has), k, v, v_first, vl, al, pk, pa, p0, pv, k2, v2, z, b, like=k)
        ctx.has = has
        ctx.dup = bool(dup)
        ctx.chain = chain
        ctx.shapes = (k_k.shape, k_a.shape, a0.shape, v0.shape if has else None)
        ctx.save_for_backward(k, v, v_first, vl, al, pk, pa, p0, pv)
        outs = (k2, v2, z, b) if has else (k2, z, b)
        if dup:                 # aliases for the second consumer (`post`): autograd then delivers their gradients separately
            outs += (k2.view_as(k2), v2.view_as(v2)) if has else (k2.view_as(k2),)
        if chain:
            outs += (v_first.view_as(v_first),)
        return outs

    @staticmethod
    def backward(ctx, *grads):
        k, v, v_first, vl, al, pk, pa, p0, pv = ctx.saved_tensors
        has = ctx.has
        n = 4 if has else 3
        dvf_in = None
        if ctx.chain:
            dvf_in, grads = grads[-1], grads[:-1]
            dvf_in = dvf_in.contiguous() if dvf_in is not None else None
        if any(g is None for g in grads):         # set_materialize_grads(False): an output nobody used
            grads = [g if g is not None else torch.zeros_like(k) for g in grads]
        main, extra = [g.contiguous() for g in grads[:n]], [g.contiguous() for g in grads[n:]]
        if has:
            dk2, dv2, dz, db = main
        else:
            dk2, dz, db = main
            dv2 = None
        dk2b = extra[0] if extra else None
        dv2b = extra[1] if len(extra) > 1 else None
        _chk(dk2, dv2, dz, db, dk2b, dv2b, dvf_in)
        C = k.shape[-1]
        ntok = k.numel() // C
        dk, dal = torch.empty_like(k), torch.empty_like(k)
        dv, dvf, dvl = [torch.empty_like(k) if has else None for _ in range(3)]
        pg, ws = _grad_rows(ntok, C, 4, k.device)
        _glue("vrwkv_kva_bwd3_bf16", ntok, C, int(has), k, v, v_first, vl, al, pk, pa, p0, pv, dk2, dv2, dz, db, dk2b, dv2b, dvf_in,
              dk, dv, dvf, dvl, dal, pg, ws, like=k)
        return (dk, dv, dvf, dvl, dal, *_rows_as(pg, k.dtype, ctx.shapes)) + (None,) * ctx.nflags          # dup, chain


class _Post(torch.autograd.Function):
    """out = (GroupNorm(y) + (sum_head r*k*r_k) * v) * g"""

    @staticmethod
    def forward(ctx, y, r, k, v, g, ln_w, ln_b, r_k, eps):
        y, r, k, v, g = [t.contiguous() for t in (y, r, k, v, g)]
        C = y.shape[-1]
        lw, lb, rk = ln_w.contiguous(), ln_b.contiguous(), r_k.reshape(C).contiguous()
        _chk(y, r, k, v, g, lw, lb, rk)
        out = torch.empty_like(y)
        _glue("vrwkv_post_fwd_bf16", y.numel() // C, C, float(eps), y, r, k, v, g, lw, lb, rk, out, like=y)
        ctx.save_for_backward(y, r, k, v, g, lw, lb, rk)
        ctx.eps = float(eps)
        ctx.rk_shape = r_k.shape
        return out

    @staticmethod
    def backward(ctx, dout):
        y, r, k, v, g, lw, lb, rk = ctx.saved_tensors
        dout = dout.contiguous()
        _chk(dout)
        C = y.shape[-1]
        dy, dr, dk, dv, dg = [torch.empty_like(y) for _ in range(5)]
        pg, ws = _grad_rows(y.numel() // C, C, 3, y.device)
        _glue("vrwkv_post_bwd_bf16", y.numel() // C, C, ctx.eps, y, r, k, v, g, lw, lb, rk, dout, dy, dr, dk, dv, dg, pg, ws, like=y)
        return dy, dr, dk, dv, dg, *_rows_as(pg, y.dtype, [(C,), (C,), ctx.rk_shape]), None


def _relusq_fwd(h):
    y = torch.empty_like(h)
    _glue("vrwkv_relusq_fwd_bf16", h.numel(), h, y, like=h)
    return y


def _relusq_bwd(h, dy):
    dh = torch.empty_like(h)
    _glue("vrwkv_relusq_bwd_bf16", h.numel(), h, dy, dh, like=h)
    return dh


class _ReluSq(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h):
        h = h.contiguous()
        _chk(h)
        ctx.save_for_backward(h)
        return _relusq_fwd(h)

    @staticmethod
    def backward(ctx, dy):
        (h,) = ctx.saved_tensors
        dy = dy.contiguous()
        _chk(dy)
        return _relusq_bwd(h, dy)


class _ReluSqLinear(torch.autograd.Function):
    """value(relu(h)^2) of the channel-mix (src/model.py:225-226) WITHOUT keeping relu(h)^2 for the backward: 4 of the ~40 activation
    tensors a layer keeps (it is as wide as the FFN).  The backward forms it again from h (one streaming kernel, 0.21 ms per layer at
    micro-batch 16) for the weight gradient.  Selective recompute (`grad_cp=2`) only; gradients are those of relu_sq + _LinearTN."""

    @staticmethod
    def forward(ctx, h, w):
        h = h.contiguous()
        _chk(h)
        ctx.save_for_backward(h, w)
        ctx.wparam = w if hasattr(w, "_vrwkv_flat_grad") else None
        return F.linear(_relusq_fwd(h), w)

    @staticmethod
    def backward(ctx, dy):
        h, w = ctx.saved_tensors
        dy = dy.contiguous()
        dw = None
        both = (ctx.needs_input_grad[0] and ctx.needs_input_grad[1]
                and _wgrad_beside_dgrad(ctx.wparam, dy.reshape(-1, dy.shape[-1]), h.reshape(-1, h.shape[-1])))
        cur = torch.cuda.current_stream(h.device)
        side = _side_stream(h.device) if both else cur
        if ctx.needs_input_grad[1]:                          # relu(h)^2 again, only for the weight gradient (on the side stream beside the input gradient: OVERLAP_WGRAD)
            if both:
                side.wait_stream(cur)
            with torch.cuda.stream(side):
                y = _relusq_fwd(h)
                dw = _weight_grad(ctx.wparam, dy.reshape(-1, dy.shape[-1]), y.reshape(-1, y.shape[-1]))
                del y
        dh = None
        if ctx.needs_input_grad[0]:
            dyy = F.linear(dy, transpose2d(w))               # gradient of relu(h)^2 (the allocator hands it the bytes just freed)
            dh = _relusq_bwd(h, dyy)
        if both:
            cur.wait_stream(side)
            dw.record_stream(cur)
        return dh, dw


mix = _Mix.apply
mix_dup3 = _MixDup3.apply
decay = _Decay.apply
kva = _Kva.apply
post = _Post.apply
relu_sq = _ReluSq.apply


def _ln_fwd_pre(who, x, delta, params, first=None):
    """What the add + LayerNorm forwards share: the inputs contiguous and checked (params: w, b and any lerp weights, each as a (C) row), `first` (the
    marks of packed rows) checked, xn -- x itself without a delta -- and the row statistics to be filled.
    Returns (x, delta, params, xn, mean, rstd)."""
    C = x.shape[-1]
    x = x.contiguous()
    delta = delta.contiguous() if delta is not None else None
    params = [p.reshape(C).contiguous() for p in params]
    _chk(x, delta, *params)
    ntok = x.numel() // C
    if first is not None and (first.dtype != torch.uint8 or first.numel() != ntok or first.device != x.device or not first.is_contiguous()):
        raise ValueError(f"{who}: `first` must be a contiguous uint8 tensor of {ntok} marks on {x.device}")
    xn = torch.empty_like(x) if delta is not None else x
    mean = torch.empty(ntok, dtype=torch.float32, device=x.device)
    rstd = torch.empty(ntok, dtype=torch.float32, device=x.device)
    return x, delta, params, xn, mean, rstd


def _add_ln_bwd(dy, d_xn, xn, mean, rstd, wc):
    """The LayerNorm's own backward (vrwkv_add_ln_bwd_bf16): (dx, dwb) = (d_xn + LN'(dy), the fp32 (dgamma, dbeta)); d_xn may be None."""
    C = xn.shape[-1]
    ntok = xn.numel() // C
    dx = torch.empty_like(xn)
    dwb = torch.empty(2, C, dtype=torch.float32, device=xn.device)
    ws = torch.empty(hip_lib.load().vrwkv_add_ln_ws_floats(ntok, C), dtype=torch.float32, device=xn.device)
    _glue("vrwkv_add_ln_bwd_bf16", ntok, C, dy, d_xn, xn, mean, rstd, wc, dx, dwb, ws, like=xn)
    return dx, dwb


def _param_grads(dwb, dmu, wc, xn, mu_shapes):
    """The fp32 parameter gradients in the parameters' dtypes and shapes: (dwb, [dmu_j])."""
    return dwb.to(wc.dtype), _rows_as(dmu, xn.dtype, mu_shapes)


class _AddLN(torch.autograd.Function):
    """(xn, y) = (x + delta, LayerNorm(x + delta));  with delta None: y = LayerNorm(x) only (csrc/ln_fused.hip)."""

    @staticmethod
    def forward(ctx, x, delta, w, b, eps):
        if delta is not None and delta.shape != x.shape:
            raise ValueError("add_ln: x and delta must have the same shape")
        x, delta, (wc, bc), xn, mean, rstd = _ln_fwd_pre("add_ln", x, delta, (w, b))
        C = x.shape[-1]
        y = torch.empty_like(x)
        _glue("vrwkv_add_ln_fwd_bf16", x.numel() // C, C, float(eps), x, delta, wc, bc, xn if delta is not None else None, y, mean, rstd, like=x)
        ctx.save_for_backward(xn, mean, rstd, wc)
        ctx.has_delta = delta is not None
        if delta is None:
            return y
        return xn, y

    @staticmethod
    def backward(ctx, *grads):
        xn, mean, rstd, wc = ctx.saved_tensors
        d_xn, dy = grads if ctx.has_delta else (None, grads[0])
        dy = dy.contiguous()
        d_xn = d_xn.contiguous() if d_xn is not None else None
        _chk(dy, d_xn)
        dx, dwb = _add_ln_bwd(dy, d_xn, xn, mean, rstd, wc)
        dwb = dwb.to(wc.dtype)
        return dx, (dx if ctx.has_delta else None), dwb[0], dwb[1], None


def add_ln(x, delta, ln):
    """Residual add + nn.LayerNorm `ln` in one kernel: returns (x + delta, ln(x + delta)); delta may be None."""
    if delta is None:
        return x, _AddLN.apply(x, None, ln.weight, ln.bias, ln.eps)
    return _AddLN.apply(x, delta, ln.weight, ln.bias, ln.eps)


@torch.no_grad()
def add_ln_infer(x, delta, dscale, ln):
    """Inference form (frozen ViT towers): returns (x + delta * dscale, LayerNorm(x + delta * dscale)); delta / dscale may be
    None.  One pass instead of the eager LayerScale multiply, residual add and LayerNorm."""
    C = x.shape[-1]
    x = x.contiguous()
    delta = delta.contiguous() if delta is not None else None
    _chk(x, delta, ln.weight, ln.bias, dscale)
    xn = torch.empty_like(x) if delta is not None else x
    y = torch.empty_like(x)
    _glue("vrwkv_add_ln_scaled_fwd_bf16", x.numel() // C, C, float(ln.eps), x, delta, dscale, ln.weight, ln.bias, xn if delta is not None else None, y,
          like=x)
    return xn, y


class _AddLnMix(torch.autograd.Function):
    """(xn, out_0 .. out_{M-1}) = (x + delta, lerps of the token-shifted LayerNorm(x + delta)): `_AddLN` followed by `_Mix` in one
    kernel each way (csrc/ln_fused.hip: ln_mix_*): the LayerNorm output is never written.  M = 1 (channel-mix) or 6 (time-mix);
    dup3: a 7th output aliasing output 3 (x_v) for its second consumer, as `_MixDup3`.  delta may be None (first block).
    first: None, or the (B*T) uint8 marks of a wkv7.PackedLayout (rows that hold several samples end to end): the _packed entries then
    shift zeros into every sample's first token and send no gradient from it to the row before.
    y_prev, want_last: x is one segment of a longer row (training across a cut; the _carry entries of csrc/ln_fused.hip / tmix_fused.hip) and
    the result is (xn, out_0 .. out_{M-1}[, alias of out_3], y_last).  y_prev (B, C), or None = zeros: the LayerNorm output of the token before
    the segment, which the shift reads at t = 0; it may require a gradient.  y_last (B, C): the LayerNorm output of the segment's last token, a
    differentiable output.  y_last is returned in fp32 (it holds bf16 values): its gradient -- the next segment's gradient of y_prev -- then
    stays fp32 between the two kernels, which add it in fp32 and round once, as they do inside a row.  Not together with `first`."""

    @staticmethod
    def forward(ctx, x, delta, w, b, eps, dup3, first, y_prev, want_last, *mus):
        B, T, C = x.shape
        M = len(mus)
        carry = want_last or y_prev is not None
        if carry and first is not None:
            raise NotImplementedError("add_ln_mix: a carry together with packed rows")
        yp = None
        if y_prev is not None:
            if tuple(y_prev.shape) != (B, C) or y_prev.device != x.device:
                raise ValueError(f"add_ln_mix: y_prev must be ({B}, {C}) on {x.device}, got {tuple(y_prev.shape)} on {y_prev.device}")
            yp = y_prev.detach().to(torch.bfloat16).contiguous()
        x, delta, (wc, bc, *mus_c), xn, mean, rstd = _ln_fwd_pre("add_ln_mix", x, delta, (w, b, *mus), first)
        _chk(yp)
        outs = [torch.empty_like(x) for _ in mus]
        y_last = torch.empty(B, C, dtype=torch.bfloat16, device=x.device) if want_last else None
        head = (B * T, T, C, float(eps), M, x, delta, wc, bc, mus_c, xn if delta is not None else None, outs, mean, rstd)
        if carry:
            _glue("vrwkv_ln_mix_fwd_carry_bf16", *head, yp, y_last, like=x)
        else:
            _glue("vrwkv_ln_mix_fwd_packed_bf16", *head, first, like=x)
        ctx.save_for_backward(xn, mean, rstd, wc, bc, *mus_c, *([yp] if yp is not None else []))
        ctx.first, ctx.carry, ctx.want_last, ctx.has_prev = first, carry, want_last, yp is not None
        ctx.prev_dtype = y_prev.dtype if y_prev is not None else None
        ctx.has_delta = delta is not None
        ctx.mu_shapes = [m.shape for m in mus]
        if dup3:
            outs.append(outs[3].view_as(outs[3]))
        return (xn, *outs, y_last.float()) if want_last else (xn, *outs)

    @staticmethod
    def backward(ctx, d_xn, *douts):
        M = len(ctx.mu_shapes)
        xn, mean, rstd, wc, bc, *rest = ctx.saved_tensors
        mus_c, yp = rest[:M], (rest[M] if ctx.has_prev else None)
        dy_last = None
        if ctx.want_last:
            *douts, dy_last = douts
            dy_last = dy_last.float().contiguous()
        B, T, C = xn.shape
        douts = [d.contiguous() for d in douts]
        d_xn = d_xn.contiguous() if d_xn is not None else None
        _chk(d_xn, *douts)
        second = douts[M] if len(douts) > M else None
        ntok = B * T
        dmu = torch.empty(M, C, dtype=torch.float32, device=xn.device)
        dy_prev = torch.empty(B, C, dtype=torch.float32, device=xn.device) if (yp is not None and ctx.needs_input_grad[7]) else None
        head = (ntok, T, C, M, xn, mean, rstd, wc, bc, mus_c, douts[:M], second)
        variant = (yp, dy_last, dy_prev) if ctx.carry else (ctx.first,)
        if M == 1:
            dx = torch.empty_like(xn)
            dwb = torch.empty(2, C, dtype=torch.float32, device=xn.device)
            ws = torch.empty(hip_lib.load().vrwkv_ln_mix_ws_floats(ntok, C, M), dtype=torch.float32, device=xn.device)
            _glue("vrwkv_ln_mix_bwd_carry_bf16" if ctx.carry else "vrwkv_ln_mix_bwd_packed_bf16", *head, d_xn, *variant, dx, dwb, dmu, ws, like=xn)
        else:       # six lerps: their backward with the LayerNorm output recomputed in place of a stored one, then the LayerNorm's
            dy = torch.empty_like(xn)
            ws = _ws(ntok, C, M, xn.device)
            _glue("vrwkv_mix_bwd_ln_carry_bf16" if ctx.carry else "vrwkv_mix_bwd_ln_packed_bf16", *head, *variant, dy, dmu, ws, like=xn)
            dx, dwb = _add_ln_bwd(dy, d_xn, xn, mean, rstd, wc)
        dwb, dmus = _param_grads(dwb, dmu, wc, xn, ctx.mu_shapes)
        return (dx, (dx if ctx.has_delta else None), dwb[0], dwb[1], None, None, None, dy_prev.to(ctx.prev_dtype) if dy_prev is not None else None, None, *dmus)


class RoutePlan:
    """Which expert every token of one batch goes through in a Block with `ffn_v` (args.modality_ffn; VisualRWKV-v7/v7.10/src/model.py:233-262), formed
    once per batch from the image mask like PackedLayout / HeadPlan and shared by all layers.
      mask  (B, T, 1) bool, as the reference passes it (already left-padded with False where the rows were padded)
      sel   (B*T) uint8 on the device: 0 = text (ffn / ln2), 1 = image (ffn_v / ln_v)
      n_v   the image-token count, a Python int: the row counts of the two experts' GEMMs are host values.  Pass it when the batch was counted on
            the host (data.DevicePrefetcher puts `n_image_tokens` into every batch before the copy to the device: no synchronisation); None
            counts the mask here, which waits for the device when the mask lives there.  A passed count is checked against the mask without
            waiting: the device-side count goes to pinned memory behind an event, like HeadPlan's, and verify() -- called by the first
            backward that uses the plan, by when the copy has long landed -- raises if the two differ (a wrong count would send rows
            through the wrong expert without any other sign)
      pos   (B*T) int32: the row of token n in the routed tensor -- image rows first, then text rows, each group in token order
      inv   (B*T) int32: the token of routed row i (the inverse of pos)
    Nothing is cached across batches."""

    def __init__(self, mask, n_v=None):
        if mask.dtype != torch.bool or mask.dim() not in (2, 3) or (mask.dim() == 3 and mask.shape[-1] != 1):
            raise ValueError(f"RoutePlan: the mask must be (B, T) or (B, T, 1) bool, got {tuple(mask.shape)} {mask.dtype}")
        self.mask = mask if mask.dim() == 3 else mask.unsqueeze(-1)
        self.B, self.T = self.mask.shape[:2]
        flat = self.mask.reshape(-1)
        self.ntok = flat.numel()
        self._pending = None
        if n_v is None or not flat.is_cuda:
            count = int(flat.sum())
            if n_v is not None and int(n_v) != count:
                raise ValueError(f"RoutePlan: n_v = {int(n_v)}, but the mask holds {count} image tokens")
            self.n_v = count
        else:
            self.n_v = int(n_v)
            host = torch.empty(1, dtype=torch.long, pin_memory=True)
            host.copy_(flat.sum().view(1), non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(flat.device))
            self._pending = (host, ev)
        if not 0 <= self.n_v <= self.ntok:
            raise ValueError(f"RoutePlan: n_v = {self.n_v} of {self.ntok} tokens")
        self.sel = flat.to(torch.uint8).contiguous()
        order = torch.argsort(~flat, stable=True)                 # image tokens first, each group in token order
        self.inv = order.to(torch.int32)
        self.pos = torch.empty_like(self.inv)
        self.pos[order] = torch.arange(self.ntok, dtype=torch.int32, device=flat.device)

    @property
    def uniform(self):
        """One expert takes every row: pos is the identity, nothing has to be brought back into token order."""
        return self.n_v == 0 or self.n_v == self.ntok

    def verify(self):
        """A caller-supplied n_v against the mask's own count (see the class docstring); waits for nothing once the copy has landed."""
        if self._pending is not None:
            host, ev = self._pending
            ev.synchronize()
            self._pending = None
            if int(host[0]) != self.n_v:
                raise ValueError(f"RoutePlan: n_v = {self.n_v} was passed in, but the mask holds {int(host[0])} image tokens: "
                                 "rows went through the wrong expert")

    def check(self, B, T, device):
        if (self.B, self.T) != (B, T) or self.sel.device != device:
            raise ValueError(f"RoutePlan: built for ({self.B}, {self.T}) on {self.sel.device}, used with ({B}, {T}) on {device}")


class _AddLnMixRouted(torch.autograd.Function):
    """`_AddLnMix` (M = 1) for a Block with two channel mixes: (xn, k_v, k_t) = (x + delta, the lerp of the image rows under (ln_v, ffn_v.x_k), of the
    text rows under (ln2, ffn.x_k)), each row through one expert, its shifted value the row before under ITS expert (csrc/ln_fused.hip:
    vrwkv_ln_mix_routed_*).  k_v (n_v, C) and k_t (ntok - n_v, C) are the two parts of one routed tensor in plan.pos order; x_k: (text, image)."""

    @staticmethod
    def forward(ctx, x, delta, w_t, b_t, w_v, b_v, eps, plan, first, mu_t, mu_v):
        B, T, C = x.shape
        plan.check(B, T, x.device)
        x, delta, params, xn, mean, rstd = _ln_fwd_pre("add_ln_mix_routed", x, delta, (w_t, w_v, b_t, b_v, mu_t, mu_v), first)
        ws, bs, mus = params[0:2], params[2:4], params[4:6]
        ntok = B * T
        out = torch.empty(ntok, C, dtype=x.dtype, device=x.device)
        _glue("vrwkv_ln_mix_routed_fwd_bf16", ntok, T, C, float(eps), x, delta, ws, bs, mus, xn if delta is not None else None, out, mean, rstd,
              first, plan.sel, plan.pos, 4, like=x)
        ctx.plan, ctx.first = plan, first
        ctx.save_for_backward(xn, mean, rstd, *ws, *bs, *mus)
        ctx.has_delta = delta is not None
        ctx.mu_shapes = (mu_t.shape, mu_v.shape)
        return xn, out[:plan.n_v], out[plan.n_v:]

    @staticmethod
    def backward(ctx, d_xn, d_kv, d_kt):
        xn, mean, rstd, w_t, w_v, b_t, b_v, mu_t, mu_v = ctx.saved_tensors
        plan = ctx.plan
        plan.verify()
        B, T, C = xn.shape
        ntok = B * T
        parts = [d for d, n in ((d_kv, plan.n_v), (d_kt, ntok - plan.n_v)) if n > 0]
        if any(d is None for d in parts):
            parts = [d if d is not None else torch.zeros(n, C, dtype=xn.dtype, device=xn.device)
                     for d, n in ((d_kv, plan.n_v), (d_kt, ntok - plan.n_v)) if n > 0]
        dout = (parts[0] if len(parts) == 1 else torch.cat(parts)).contiguous()
        d_xn = d_xn.contiguous() if d_xn is not None else None
        _chk(d_xn, dout)
        dx = torch.empty_like(xn)
        dwb = torch.empty(2, 2, C, dtype=torch.float32, device=xn.device)
        dmu = torch.empty(2, C, dtype=torch.float32, device=xn.device)
        ws = torch.empty(hip_lib.load().vrwkv_ln_mix_routed_ws_floats(ntok, C), dtype=torch.float32, device=xn.device)
        _glue("vrwkv_ln_mix_routed_bwd_bf16", ntok, T, C, xn, mean, rstd, [w_t, w_v], [b_t, b_v], [mu_t, mu_v], dout, d_xn, ctx.first, plan.sel, plan.pos, 4,
              dx, dwb, dmu, ws, like=xn)
        dwb, dmus = _param_grads(dwb, dmu, w_t, xn, ctx.mu_shapes)
        return (dx, (dx if ctx.has_delta else None), dwb[0, 0], dwb[0, 1], dwb[1, 0], dwb[1, 1], None, None, None, *dmus)


def row_gather(src, idx):
    """src[idx] for (n, C) bf16 rows and an int32 / int64 index on the device (csrc/ln_fused.hip: vrwkv_row_gather_bf16); no autograd."""
    src = src.contiguous()
    _chk(src)
    n, C = idx.numel(), src.shape[-1]
    out = torch.empty(n, C, dtype=src.dtype, device=src.device)
    _glue("vrwkv_row_gather_bf16", n, C, src, idx, idx.element_size(), out, like=src)
    return out


class _Unroute(torch.autograd.Function):
    """The routed tensor (rows in plan.pos order) back in token order: out[n] = routed[pos[n]]; the gradient goes the other way through plan.inv."""

    @staticmethod
    def forward(ctx, routed, plan):
        ctx.plan = plan
        return row_gather(routed, plan.pos)

    @staticmethod
    def backward(ctx, d):
        return row_gather(d.reshape(-1, d.shape[-1]), ctx.plan.inv), None


def add_ln_mix_routed(x, delta, ln_t, ln_v, x_k_t, x_k_v, plan, first=None):
    """Returns (x + delta, k_v, k_t) -- see `_AddLnMixRouted`."""
    if ln_t.eps != ln_v.eps:
        raise ValueError("add_ln_mix_routed: ln2 and ln_v must share eps (the row statistics are computed once)")
    return _AddLnMixRouted.apply(x, delta, ln_t.weight, ln_t.bias, ln_v.weight, ln_v.bias, ln_t.eps, plan, first, x_k_t, x_k_v)


def cmix_routed(block, x, att_out, plan, first=None, selective=False):
    """The end of a Block with `ffn_v`: x + att_out, then where(mask, ffn_v(ln_v(.)), ffn(ln2(.))) with every row through its own expert only --
    one routed add_ln_mix, the two channel mixes on n_v and ntok - n_v rows, and one pass back into token order.  Returns (x + att_out, the
    channel-mix output still to be added)."""
    B, T, C = x.shape
    x, k_v, k_t = add_ln_mix_routed(x, att_out, block.ln2, block.ln_v, block.ffn.x_k, block.ffn_v.x_k, plan, first)
    parts = []
    if plan.n_v > 0:
        parts.append(cmix_from_mixed(block.ffn_v, k_v, recompute_relusq=selective))
    if plan.n_v < plan.ntok:
        parts.append(cmix_from_mixed(block.ffn, k_t, recompute_relusq=selective))
    if plan.uniform:
        return x, parts[0].view(B, T, C)
    return x, _Unroute.apply(torch.cat(parts), plan).view(B, T, C)


def add_ln_mix(x, delta, ln, mus, dup3=False, first=None, carry=None):
    """Returns (x + delta, [lerp outputs]) -- see `_AddLnMix`.  first: the marks of a wkv7.PackedLayout (layout.first) for packed rows.
    carry: a 1-tuple (y_prev,) when x is one segment of a longer row (y_prev may be None: the row starts here); returns
    (x + delta, [lerp outputs], y_last) then."""
    if carry is not None:
        if first is not None:
            raise NotImplementedError("add_ln_mix: a carry together with packed rows")
        xn, *outs, y_last = _AddLnMix.apply(x, delta, ln.weight, ln.bias, ln.eps, dup3, None, carry[0], True, *mus)
        return xn, outs, y_last
    xn, *outs = _AddLnMix.apply(x, delta, ln.weight, ln.bias, ln.eps, dup3, first, None, False, *mus)
    return xn, outs


def packed_supported(x):
    """May a packed batch (wkv7.PackedLayout) take blocks_forward?  It needs both shifts inside the ln_mix kernels: the two-kernel shift
    (vrwkv_mix_fwd / _bwd, the path for C > 4096 and for input that is not 3-D) finds a first token as n % T == 0 only; the caller runs the
    unfused Blocks then."""
    return ln_mix_supported(x)


def carry_supported(x):
    """May one segment of a cut row (rwkv7.TrainCarry) take blocks_forward?  As for packed rows, both shifts must be inside the ln_mix kernels;
    the caller runs the unfused Blocks otherwise."""
    return ln_mix_supported(x)


def ln_mix_supported(x):
    return add_ln_supported(x) and x.dim() == 3 and x.shape[-1] <= 4096


def add_ln_supported(x):
    return x.is_cuda and x.dtype == torch.bfloat16 and x.shape[-1] % 64 == 0 and x.shape[-1] <= 8192


def _block_segment(block, x, delta, v_first, selective=False, layout=None, carry=None, route=None):
    """One Block on the (x, pending delta) residual stream: returns (x + delta, ffn output still to be added, v_first).
    route: a RoutePlan when the Block has `ffn_v` / `ln_v` (args.modality_ffn): image rows take those, text rows ffn / ln2 (cmix_routed).
    selective: the selective-recompute mode of blocks_forward (WKV7 by-products and relu(h)^2 are re-formed in the backward).
    layout: a wkv7.PackedLayout -- both token shifts and the WKV7 state restart at every sample of a row (packed_supported(x) must hold).
    carry: this layer's (att_x, ffn_x, S) of a rwkv7.TrainCarry (x is one segment of a longer row; carry_supported(x) must hold): the result
    gains the layer's next carry (att_x, ffn_x, S) as three more entries."""
    att, ffn = block.att, block.ffn
    fuse = ln_mix_supported(x) and getattr(att.args, "fused", False)
    if (route is None) != (getattr(block, "ffn_v", None) is None):
        raise ValueError("a Block with ffn_v needs the image mask (a RoutePlan), a Block without one takes none")
    if carry is not None and route is not None:
        raise NotImplementedError("a training carry together with modality routing: the carried channel-mix row would have to be re-normed per expert")
    if carry is not None:
        if layout is not None:
            raise NotImplementedError("a training carry together with packed rows")
        if not fuse:
            raise NotImplementedError("a cut row needs the fused ln_mix kernels for both token shifts (fused.carry_supported)")
        dup3 = torch.is_grad_enabled() and GRAD_ALIAS and att.layer_id > 0
        x, mixed, att_x = add_ln_mix(x, delta, block.ln1, (att.x_r, att.x_w, att.x_k, att.x_v, att.x_a, att.x_g), dup3, None, (carry[0],))
        att_out, v_first, s_end = tmix_from_mixed(att, mixed, v_first, recompute_state=selective, state0=carry[2], want_state=True)
        x, (k,), ffn_x = add_ln_mix(x, att_out, block.ln2, (ffn.x_k,), False, None, (carry[1],))
        return x, cmix_from_mixed(ffn, k, recompute_relusq=selective), v_first, att_x, ffn_x, s_end
    first = layout.first if layout is not None else None
    if layout is not None and not fuse:
        raise NotImplementedError("packed rows need the fused ln_mix kernels for both token shifts (fused.packed_supported)")
    if fuse:
        dup3 = torch.is_grad_enabled() and GRAD_ALIAS and att.layer_id > 0
        x, mixed = add_ln_mix(x, delta, block.ln1, (att.x_r, att.x_w, att.x_k, att.x_v, att.x_a, att.x_g), dup3, first)
        att_out, v_first = tmix_from_mixed(att, mixed, v_first, recompute_state=selective, layout=layout)
    else:
        x, h = add_ln(x, delta, block.ln1)
        att_out, v_first = tmix_forward(att, h, v_first, recompute_state=selective) if getattr(att.args, "fused", False) else att(h, v_first)
    if fuse and route is not None:
        x, out = cmix_routed(block, x, att_out, route, first, selective)
        return x, out, v_first
    if fuse:            # ln2 + the channel-mix lerp in one kernel: the LayerNorm output is never materialised
        x, (k,) = add_ln_mix(x, att_out, block.ln2, (ffn.x_k,), False, first)
        return x, cmix_from_mixed(ffn, k, recompute_relusq=selective), v_first
    x, h = add_ln(x, att_out, block.ln2)
    if route is not None:       # no ln_mix kernels for this shape: the reference's statement, both channel mixes on every row
        return x, torch.where(route.mask, block.ffn_v(block.ln_v(x)), ffn(h)), v_first
    return x, ffn(h), v_first


def _block_segment_carry(block, x, delta, v_first, selective, att_x, ffn_x, S):
    """_block_segment with the carry tensors as arguments of their own: what blocks_forward's mode 1 checkpoints."""
    return _block_segment(block, x, delta, v_first, selective, None, (att_x, ffn_x, S))


def blocks_forward(rwkv, x, grad_cp=0, layout=None, carry=None, route=None):
    """All Blocks + ln_out with the residual adds fused into the LayerNorms (same math as Block.forward chained,
    src/model.py:247-254,313-318): the residual stream is carried as (x, pending delta).
    grad_cp (the reference's memory-saving switch, src/model.py:318-319: deepspeed.checkpointing.checkpoint per block):
      0  keep every activation (288 GB of HBM hold the 1.5B model at micro-batch 16: 192 GB);
      1  THE REFERENCE'S RECIPE, same memory behaviour: every Block re-computed in the backward (block inputs only are kept: 42 GB) -- through
         these same fused kernels, so the recompute and the backward use add_ln / the glue kernels / the WKV7 op, not the eager modules;
      2  (not in the reference) SELECTIVE recompute: keep what is expensive to recompute (every GEMM output), drop what is cheap to recompute and
         large -- the WKV7 chunk checkpoints `s` and `sa` (10 of the ~40 activation tensors of a layer: the backward re-runs the forward kernel)
         and relu(h)^2 of the channel-mix (4 of them: one streaming kernel) -- about a third of the activation memory for ~1 ms per layer.
    (Rounds 4-5 had 1 and 2 the other way round; a trainer configured for the reference's `--grad_cp 1` must not get the mode that needs 3x
    the memory.)
    layout: a wkv7.PackedLayout when the rows hold several samples end to end; every mode passes it to every Block.
    carry: a rwkv7.TrainCarry when x is one segment of a longer row; every mode threads it through every Block (mode 1 checkpoints the Block
    with the carry tensors among its arguments, mode 2 lets the WKV7 state op regenerate its by-products from the carried state) and the
    result is (hidden, the carry leaving the segment).
    route: a RoutePlan when the Blocks have `ffn_v` (args.modality_ffn); every mode passes it to every Block.  Not together with a carry."""
    x, delta, layers = _blocks_walk(rwkv, x, grad_cp, layout, carry, route)
    _, h = add_ln(x, delta, rwkv.ln_out)
    if carry is not None:
        from .rwkv7 import TrainCarry
        return h, TrainCarry(len(layers), layers)
    return h


def _blocks_walk(rwkv, x, grad_cp=0, layout=None, carry=None, route=None):
    """blocks_forward up to (not including) ln_out, on any module with `blocks` (Block 0 owns ln0): returns (x, pending delta, the per-layer
    carries leaving the segment), so that a caller can fold the last residual add into its own tail kernel (vrwkv_forward)."""
    grad_cp = int(grad_cp) if torch.is_grad_enabled() else 0
    if grad_cp not in (0, 1, 2):
        raise ValueError(f"grad_cp = {grad_cp}: 0 (keep everything), 1 (re-compute every block, the reference's recipe) or 2 (selective recompute)")
    if carry is not None and layout is not None:
        raise NotImplementedError("a training carry together with packed rows")
    if carry is not None and route is not None:
        raise NotImplementedError("a training carry together with modality routing (cut rows are not routed)")
    if route is not None:
        route.check(x.shape[0], x.shape[1], x.device)
    x = rwkv.blocks[0].ln0(x)
    v_first = torch.empty_like(x)
    delta = None
    layers = []
    for i, block in enumerate(rwkv.blocks):
        if carry is not None:
            if grad_cp == 1:
                from torch.utils.checkpoint import checkpoint
                x, delta, v_first, *lc = checkpoint(_block_segment_carry, block, x, delta, v_first, False, *carry[i], use_reentrant=False)
            else:
                x, delta, v_first, *lc = _block_segment(block, x, delta, v_first, grad_cp == 2, None, carry[i])
            layers.append(tuple(lc))
        elif grad_cp == 1:
            from torch.utils.checkpoint import checkpoint
            x, delta, v_first = checkpoint(_block_segment, block, x, delta, v_first, False, layout, None, route, use_reentrant=False)
        else:
            x, delta, v_first = _block_segment(block, x, delta, v_first, grad_cp == 2, layout, None, route)
    return x, delta, layers


class _FusedCE(torch.autograd.Function):
    """training_step's loss (shifted CE, per-sample sum / max(valid,1), batch mean) with L2Wrap's gradient term
    (src/model.py:418-434,257-271) -- csrc/loss_fused.hip."""

    @staticmethod
    def forward(ctx, logits, targets, ignore_index):
        B, T, V = logits.shape
        logits = logits.contiguous()
        _chk(logits)
        labels = torch.full((B, T), ignore_index, dtype=torch.long, device=logits.device)
        labels[:, :-1] = targets[:, 1:]                       # row (b,t) predicts token t+1; the last row has no target
        labels = torch.where(labels == ignore_index, torch.full_like(labels, -100), labels)
        valid = (labels >= 0).sum(1).clamp(min=1)
        n = B * T
        dev = logits.device
        row_loss, row_max, row_lse = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(3))
        row_arg = torch.empty(n, dtype=torch.int32, device=dev)
        _glue("vrwkv_ce_fwd_bf16", n, V, logits, labels, row_loss, row_max, row_lse, row_arg, like=logits)
        w = ((labels >= 0).float() / (valid.float().unsqueeze(1) * B)).view(n)      # d loss / d row_loss
        ctx.save_for_backward(logits, labels, w, row_max, row_lse, row_arg)
        return (row_loss * w).sum().to(logits.dtype)

    @staticmethod
    def backward(ctx, g):
        logits, labels, w, row_max, row_lse, row_arg = ctx.saved_tensors
        B, T, V = logits.shape
        dlogits = torch.empty_like(logits)
        row_w = (w * g.float()).contiguous()
        _glue("vrwkv_ce_bwd_bf16", B * T, V, logits, labels, row_w, row_max, row_lse, row_arg, 1e-4 / (B * T), dlogits, like=logits)
        return dlogits, None, None


def loss_from_logits(logits, targets, ignore_index=-100):
    return _FusedCE.apply(logits, targets, ignore_index)


def ce_supported(logits):
    return logits.is_cuda and logits.dtype == torch.bfloat16 and logits.dim() == 3 and logits.shape[-1] % 8 == 0


# Head + loss as one node whose backward runs the dense part on the labelled rows only (DESIGN.md "The head's backward on labelled rows").
# A row without a label has one nonzero logit gradient (L2Wrap's c = bf16(max * 1e-4/(B*T)) at its arg-max): its input gradient is c W[arg]
# and its weight gradient c x added to W's row arg, both from csrc/loss_fused.hip.  The two head GEMMs and the CE backward run over the
# labelled rows, padded to HEAD_ROW_ALIGN (one tuned shape per labelled count of the batch).  0 = linear + _FusedCE (dense over every row).
HEAD_COMPACT = os.environ.get("VRWKV_HEAD_COMPACT", "1") != "0"
HEAD_ROW_ALIGN = 256
# above this labelled fraction the dense backward is used: the compact path saves GEMM rows in proportion to the unlabelled share and
# costs a few hundred us of its own (gather, sort, dx assembly, sparse weight gradient); the two meet at 0.95 at the bench shape
# (profiles/r7_head_compact_micro.jsonl)
HEAD_COMPACT_MAX_FRACTION = 0.9


class HeadPlan:
    """The labelled rows of one batch, formed at the start of training_step from the labels alone: the shifted labels and per-row loss
    weights of _FusedCE, and the count of labelled rows copied to pinned host memory behind an event -- by the head's backward the copy has
    long landed, so reading it waits for nothing (no device-wide synchronisation in the step).  Rows are those of the hidden state left-padded
    by `pad` rows per sample (RWKV.forward_features): pad rows carry no label and get no gradient.  Nothing is cached across batches.
    layout (a wkv7.PackedLayout; pad is 0 then): "sample" means segment of a packed row -- the last row of a segment has no target, and a
    labelled row weighs 1 / (valid labels of its segment * layout.n_samples).
    window = (a, b) (train_step_cut; pad is 0, no layout): the plan describes rows a .. b-1 of the (B, T) row `targets` -- the hidden state it
    goes with is (B, b-a, C).  Labels and weights are the whole row's: row b-1 predicts token b of the row, a labelled row weighs
    1 / (valid labels of its whole sample * B), and `l2_rows` (L2Wrap's B * T) counts the whole row, so that the windows' losses add up to
    the loss of the uncut row."""

    def __init__(self, targets, pad, ignore_index=-100, layout=None, window=None):
        B, T = targets.shape
        dev = targets.device
        labels = torch.full((B, T), ignore_index, dtype=torch.long, device=dev)
        labels[:, :-1] = targets[:, 1:]                       # row (b,t) predicts token t+1; the last row has no target
        labels = torch.where(labels == ignore_index, torch.full_like(labels, -100), labels)
        if layout is None:
            valid = (labels >= 0).sum(1).clamp(min=1)
            self.w = ((labels >= 0).float() / (valid.float().unsqueeze(1) * B)).view(B * T)      # _FusedCE's d loss / d row_loss
        else:
            if pad != 0:
                raise ValueError("HeadPlan: packed rows are whole chunks, pad must be 0")
            layout.check(B, T, dev)
            labels[:, :-1] = labels[:, :-1].masked_fill(layout.first.view(B, T)[:, 1:].bool(), -100)      # the next token opens another sample
            lab = (labels >= 0).float().view(-1)
            seg = layout.seg_id.view(-1).long()
            valid = torch.zeros(layout.n_segments, dtype=torch.float32, device=dev).index_add_(0, seg, lab).clamp_(min=1)
            self.w = lab / (valid[seg] * layout.n_samples)
        self.l2_rows = B * T
        if window is not None:
            a, b_ = window
            if layout is not None or pad != 0 or not (0 <= a < b_ <= T):
                raise ValueError(f"HeadPlan: a window needs pad 0, no layout and 0 <= a < b <= T (got {window}, pad {pad})")
            labels = labels[:, a:b_].contiguous()
            self.w = self.w.view(B, T)[:, a:b_].reshape(-1)
            T = b_ - a
        self.B, self.T, self.pad = B, T, pad
        Tp = T + pad
        lab_p = torch.full((B, Tp), -100, dtype=torch.long, device=dev)
        lab_p[:, pad:] = labels
        self.labels = lab_p.view(B * Tp)                      # padded layout: what the kernels index
        mask = self.labels >= 0
        count = mask.sum()
        self.n_host = torch.empty(1, dtype=torch.long, pin_memory=True)
        self.n_host.copy_(count.view(1), non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record(torch.cuda.current_stream(dev))
        self.count = count
        self.order = torch.argsort(~mask, stable=True)         # labelled rows first, ascending
        real = torch.zeros(B, Tp, dtype=torch.bool, device=dev)
        real[:, pad:] = True
        # pos: compact slot of a labelled row, -1 for a row without a label, -2 for a pad row
        self.pos = torch.where(mask, torch.cumsum(mask, 0) - 1, torch.where(real.view(-1), -1, -2))
        self._n = None

    def n_labelled(self):
        if self._n is None:
            self.event.synchronize()
            self._n = int(self.n_host[0])
        return self._n

    def idx(self, nrows):
        """Source row of each of the nrows compact rows: the labelled rows in order, then -1."""
        n = self.order.numel()
        idx = torch.full((nrows,), -1, dtype=torch.long, device=self.order.device)
        k = min(nrows, n)
        idx[:k] = torch.where(torch.arange(k, device=idx.device) < self.count, self.order[:k], -1)
        return idx


def head_loss_supported(head, labels, x=None):
    """May training_step take head + loss through _HeadCE?  `x`: the hidden state, once it exists."""
    w = head.weight
    return (HEAD_COMPACT and torch.is_grad_enabled() and labels.is_cuda and w.is_cuda and w.dtype == torch.bfloat16 and head.bias is None
            and w.dim() == 2 and w.shape[0] % 8 == 0 and w.shape[1] % 8 == 0
            and (x is None or (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 3 and x.shape[-1] == w.shape[1])))


class _HeadCE(torch.autograd.Function):
    """loss_from_logits(unpad(linear(head, x))) for the left-padded hidden state x (B, T+pad, C) -- the same forward GEMM over the same
    rows and the same CE kernel, so the loss is bit-identical.  Backward: ce_bwd on the labelled rows into a compact gradient, the input
    gradient of those rows from one library GEMM, c W[arg] for the others (head_dx), the weight gradient of the labelled rows from one
    library GEMM into the ZeRO-1 slot (_weight_grad) plus the sparse L2Wrap rows (l2wrap_wgrad).  The GEMMs run one after the other.
    Above HEAD_COMPACT_MAX_FRACTION labelled rows the backward is the dense one of linear + _FusedCE, over every row, with the same
    kernels and GEMM shapes."""

    @staticmethod
    def forward(ctx, x, w, plan):
        x = x.contiguous()
        _chk(x, w)
        B, Tp, C = x.shape
        if B != plan.B or Tp != plan.T + plan.pad:
            raise ValueError(f"head_loss: hidden state {tuple(x.shape)} does not match the plan ({plan.B}, {plan.T} + {plan.pad})")
        logits = F.linear(x, w)
        V = logits.shape[-1]
        n = B * Tp
        dev = x.device
        row_loss, row_max, row_lse = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(3))
        row_arg = torch.empty(n, dtype=torch.int32, device=dev)
        _glue("vrwkv_ce_fwd_bf16", n, V, logits, plan.labels, row_loss, row_max, row_lse, row_arg, like=logits)
        ctx.save_for_backward(x, w, logits, row_max, row_lse, row_arg)
        ctx.plan = plan
        ctx.wparam = w if hasattr(w, "_vrwkv_flat_grad") else None
        return (row_loss.view(B, Tp)[:, plan.pad:].reshape(-1) * plan.w).sum().to(logits.dtype)

    @staticmethod
    def backward(ctx, g):
        x, w, logits, row_max, row_lse, row_arg = ctx.saved_tensors
        plan = ctx.plan
        B, Tp, C = x.shape
        V = w.shape[0]
        N, n_real = B * Tp, B * plan.T
        dev = x.device
        row_w = torch.zeros(B, Tp, dtype=torch.float32, device=dev)
        row_w[:, plan.pad:] = (plan.w * g.float()).view(B, plan.T)      # _FusedCE's row_w on the real rows, 0 on the pad rows
        row_w = row_w.view(N)
        l2f = 1e-4 / plan.l2_rows                                        # = n_real, except for a window of a longer row
        x2 = x.view(N, C)
        n_lab = plan.n_labelled()
        compact = n_lab <= HEAD_COMPACT_MAX_FRACTION * n_real
        if compact:
            nrows = -(-n_lab // HEAD_ROW_ALIGN) * HEAD_ROW_ALIGN
            idx = plan.idx(nrows)
        else:                                                            # every real row dense: linear + _FusedCE's backward
            nrows = N
            idx = torch.where(plan.pos >= -1, torch.arange(N, device=dev), -1)
        dlog = torch.empty(nrows, V, dtype=torch.bfloat16, device=dev)
        if nrows:
            _glue("vrwkv_ce_bwd_rows_bf16", nrows, V, logits, plan.labels, row_w, row_max, row_lse, row_arg, l2f, idx, dlog, like=x)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dxc = F.linear(dlog, transpose2d(w)) if nrows else torch.empty(0, C, dtype=x.dtype, device=dev)
            if compact:
                dx = torch.empty(N, C, dtype=x.dtype, device=dev)
                _glue("vrwkv_head_dx_bf16", N, C, plan.pos, dxc, w, row_max, row_arg, l2f, dx, like=x)
            else:
                dx = dxc
            dx = dx.view(B, Tp, C)
        if ctx.needs_input_grad[1]:
            xl = x2.index_select(0, idx.clamp(min=0)) if compact else x2      # compact padding rows: any row (its gradient row is 0)
            dw = _weight_grad(ctx.wparam, dlog, xl)
            n_u = n_real - n_lab
            if compact and n_u > 0:
                key = torch.where(plan.pos == -1, row_arg.long(), V)
                srow = torch.sort(key, stable=True).indices[:n_u].contiguous()
                ws = torch.empty(hip_lib.load().vrwkv_l2wrap_wgrad_ws_floats(n_u, C), dtype=torch.float32, device=dev)
                _glue("vrwkv_l2wrap_wgrad_bf16", n_u, C, srow, x2, row_max, row_arg, l2f, dw, ws, like=x)
        return dx, dw, None


def head_loss(head, x, plan):
    """training_step's loss from the left-padded hidden state x = RWKV.forward_features(...)[0]: _HeadCE (see there)."""
    return _HeadCE.apply(x, head.weight, plan)


# ---------------------------------------------------------------------------------------------------------------
# RWKV-6 glue (BASELINE config 4; VisualRWKV-v6/v6.0/src/model.py:146-194, 213-226)
# ---------------------------------------------------------------------------------------------------------------
class _DDMix(torch.autograd.Function):
    """RWKV-6's data-dependent token shift: out_j = x + (shift(x) - x) * (mu_j + mm_j), j < 5, mm_j (B,T,C) per token."""

    @staticmethod
    def forward(ctx, x, mm, *mus):
        B, T, C = x.shape
        x = x.contiguous()
        mm = mm.contiguous()                                # (5, B, T, C)
        mus_c = [m.reshape(C).contiguous() for m in mus]
        _chk(x, mm, *mus_c)
        assert len(mus) == 5 and tuple(mm.shape) == (5, B, T, C)
        outs = [torch.empty_like(x) for _ in range(5)]
        _glue("vrwkv_ddmix_fwd_bf16", B * T, T, C, x, mus_c, mm.unbind(0), outs, like=x)
        ctx.save_for_backward(x, mm, *mus_c)
        ctx.mu_shapes = [m.shape for m in mus]
        return tuple(outs)

    @staticmethod
    def backward(ctx, *douts):
        x, mm, *mus_c = ctx.saved_tensors
        B, T, C = x.shape
        douts = [d.contiguous() for d in douts]
        _chk(*douts)
        dx, dmm = torch.empty_like(x), torch.empty_like(mm)
        dmu, ws = _grad_rows(B * T, C, 5, x.device)
        _glue("vrwkv_ddmix_bwd_bf16", B * T, T, C, x, mus_c, mm.unbind(0), douts, dx, dmm.unbind(0), dmu, ws, like=x)
        return (dx, dmm, *_rows_as(dmu, x.dtype, ctx.mu_shapes))


class _GnSilu(torch.autograd.Function):
    """out = GroupNorm(C/64 groups)(y) * silu(gg)   (RWKV_Tmix_x060.jit_func_2 with the silu of jit_func)"""

    @staticmethod
    def forward(ctx, y, gg, ln_w, ln_b, eps):
        y, gg = y.contiguous(), gg.contiguous()
        C = y.shape[-1]
        lw, lb = ln_w.contiguous(), ln_b.contiguous()
        _chk(y, gg, lw, lb)
        out = torch.empty_like(y)
        _glue("vrwkv_gn_silu_fwd_bf16", y.numel() // C, C, float(eps), y, gg, lw, lb, out, like=y)
        ctx.save_for_backward(y, gg, lw, lb)
        ctx.eps = float(eps)
        return out

    @staticmethod
    def backward(ctx, dout):
        y, gg, lw, lb = ctx.saved_tensors
        dout = dout.contiguous()
        _chk(dout)
        C = y.shape[-1]
        dy, dgg = torch.empty_like(y), torch.empty_like(gg)
        pg, ws = _grad_rows(y.numel() // C, C, 2, y.device)
        _glue("vrwkv_gn_silu_bwd_bf16", y.numel() // C, C, ctx.eps, y, gg, lw, lb, dout, dy, dgg, pg, ws, like=y)
        return dy, dgg, *_rows_as(pg, y.dtype, [(C,), (C,)]), None


ddmix = _DDMix.apply
gn_silu = _GnSilu.apply


def supported6(x, m=None):
    """bf16 CUDA activations with C a multiple of 64 (the glue kernels' 8-channel lanes and 64-channel heads).  With the time-mix
    module `m`: its GroupNorm must be the 64-channel-per-head one over all C channels that gn_silu hard-codes (head_size 64,
    dim_att == n_embd); anything else takes the eager path."""
    ok = x.is_cuda and x.dtype == torch.bfloat16 and x.shape[-1] % 64 == 0 and x.shape[-1] <= 8192
    if ok and m is not None and hasattr(m, "ln_x"):
        ok = getattr(m, "head_size", 64) == 64 and m.ln_x.num_groups * 64 == x.shape[-1] == m.ln_x.num_channels
    return ok


_NO_STATE = object()


def tmix6_forward(m, x, wkv=None, state=_NO_STATE, want_state=True):
    """RWKV_Tmix_x060.forward (VisualRWKV-v6/v6.0/src/model.py:146-194) with the glue fused: one kernel for the first lerp
    (xxx), one for the five data-dependent lerps, the T,N input-gradient layout for the projections, GroupNorm * silu(gate)
    in one pass.  `m` is the module (parameter names as in the reference).  With `state` given (a (B,H,64,64) f32 [key][value]
    tensor, or None for zeros) this is RWKV_Tmix_x060_state.forward of v6.xx (model.py:137-144): the WKV starts from it and
    (out, final state) is returned; `wkv` then has RUN_CUDA_RWKV6_STATE's signature, and want_state=False (product op only)
    leaves the final state unwritten and returns None for it."""
    from . import wkv6 as _wkv6
    B, T, C = x.shape
    mm_ = lora_mm if torch.is_grad_enabled() and LORA_WGRAD else torch.matmul
    (xxx,) = mix(x, m.time_maa_x)
    h = torch.tanh(mm_(xxx, m.time_maa_w1)).view(B * T, 5, -1).transpose(0, 1)
    mm5 = torch.bmm(h, m.time_maa_w2).view(5, B, T, C)
    xw, xk, xv, xr, xg = ddmix(x, mm5, m.time_maa_w, m.time_maa_k, m.time_maa_v, m.time_maa_r, m.time_maa_g)
    r = linear(m.receptance, xr)
    k = linear(m.key, xk)
    v = linear(m.value, xv)
    gg = linear(m.gate, xg)
    w = m.time_decay + mm_(torch.tanh(mm_(xw, m.time_decay_w1)), m.time_decay_w2)
    if state is _NO_STATE:
        run = wkv if wkv is not None else _wkv6.RUN_CUDA_RWKV6
        y = run(B, T, C, m.n_head, r, k, v, w, m.time_faaaa)
    elif wkv is not None:
        y, state = wkv(B, T, C, m.n_head, r, k, v, w, m.time_faaaa, state)
    else:
        y, state = _wkv6.RUN_CUDA_RWKV6_STATE(B, T, C, m.n_head, r, k, v, w, m.time_faaaa, state, want_state)
    y = gn_silu(y.reshape(B * T, C), gg.reshape(B * T, C), m.ln_x.weight, m.ln_x.bias, m.ln_x.eps).view(B, T, C)
    out = linear(m.output, y)
    return out if state is _NO_STATE else (out, state)


def cmix6_forward(m, x):
    """RWKV_CMix_x060.forward (model.py:213-226): two lerps in one pass, relu^2, sigmoid(receptance) * value in one pass."""
    xk, xr = mix(x, m.time_maa_k, m.time_maa_r)
    kv = linear(m.value, relu_sq(linear(m.key, xk)))
    return gate(kv, linear(m.receptance, xr))


def blocks6_forward(rwkv, x, wkv=None, grad_cp=False):
    """RWKV-6 Blocks + ln_out with the residual adds fused into the LayerNorms (model.py:233-258,300-325)."""
    x = rwkv.blocks[0].ln0(x)
    delta = None

    def seg(block, x, delta):
        x, h = add_ln(x, delta, block.ln1)
        x, h = add_ln(x, tmix6_forward(block.att, h, wkv), block.ln2)
        return x, cmix6_forward(block.ffn, h)

    for block in rwkv.blocks:
        if grad_cp:
            from torch.utils.checkpoint import checkpoint
            x, delta = checkpoint(seg, block, x, delta, use_reentrant=False)
        else:
            x, delta = seg(block, x, delta)
    _, h = add_ln(x, delta, rwkv.ln_out)
    return h


def blocks6_forward_state(rwkv, x, x_emb, wkv=None, grad_cp=False):
    """The Block loop of v6.xx's unidirectional_forward + ln_out (VisualRWKV-v6/v6.xx/src/model.py:326-341) on the fused glue: the
    (x, delta) residual stream is carried twice per Block -- first over the projected image features `x_emb` from a zero WKV state,
    keeping the state that pass ends in, then over the text `x` from that state (its own final state is not requested).  ln0 of
    Block 0 applies to both streams (the reference's Block applies it on every call); ln_out runs on the text only.  grad_cp
    checkpoints the two passes of a Block separately, as model.py:334-336 does."""
    ln0 = rwkv.blocks[0].ln0
    x, e = ln0(x), ln0(x_emb)
    dx = de = None

    def seg(block, x, delta, state, want_state):
        x, h = add_ln(x, delta, block.ln1)
        a, state = tmix6_forward(block.att, h, wkv, state=state, want_state=want_state)
        x, h = add_ln(x, a, block.ln2)
        return x, cmix6_forward(block.ffn, h), state

    for block in rwkv.blocks:
        if grad_cp:
            from torch.utils.checkpoint import checkpoint
            e, de, state = checkpoint(seg, block, e, de, None, True, use_reentrant=False)
            x, dx, _ = checkpoint(seg, block, x, dx, state, False, use_reentrant=False)
        else:
            e, de, state = seg(block, e, de, None, True)
            x, dx, _ = seg(block, x, dx, state, False)
    _, h = add_ln(x, dx, rwkv.ln_out)
    return h


def tmix_forward(m, x, v_first, recompute_state=False, layout=None):
    """RWKV_Tmix_x070.forward (src/model.py:163-195) with the glue fused; `m` is the module.  Its own shift kernel (vrwkv_mix_fwd) knows no
    sample boundaries inside a row: packed rows come through add_ln_mix + tmix_from_mixed (blocks_forward)."""
    if layout is not None:
        raise NotImplementedError("tmix_forward: packed rows take their token shift in add_ln_mix (fused.blocks_forward), not in the two-kernel path")
    train = torch.is_grad_enabled()
    if train and GRAD_ALIAS and m.layer_id > 0:          # x_v, k2, v2 have two consumers each: aliases keep their gradients apart until the
        mixed = mix_dup3(x, m.x_r, m.x_w, m.x_k, m.x_v, m.x_a, m.x_g)      # backward kernels sum them
    else:
        mixed = mix(x, m.x_r, m.x_w, m.x_k, m.x_v, m.x_a, m.x_g)
    return tmix_from_mixed(m, mixed, v_first, recompute_state)


def tmix_from_mixed(m, mixed, v_first, recompute_state=False, layout=None, state0=None, want_state=False):
    """The time-mix after its token shift: `mixed` = (xr, xw, xk, xv, xa, xg[, alias of xv for its second consumer]).
    layout: a wkv7.PackedLayout -- the WKV7 op restarts its state at every sample of a row (one packed launch each way).
    want_state (one segment of a cut row): the recurrence runs through the state op from state0 (B,H,64,64) fp32 -- None: the layer's tuned
    state, else zeros -- and the state after the last token is returned as a third result; gradients flow through both."""
    xr, xw, xk, xv, xa, xg = mixed[:6]
    xv_b = mixed[6] if len(mixed) > 6 else xv
    mm = lora_mm if torch.is_grad_enabled() and LORA_WGRAD else torch.matmul     # training: skinny weight-gradient kernel in the backward
    r, k, v = linear3((m.receptance, m.key, m.value), (xr, xk, xv))
    w = decay(mm(torch.tanh(mm(xw, m.w1)), m.w2), m.w0)
    al = mm(mm(xa, m.a1), m.a2)
    g = mm(torch.sigmoid(mm(xg, m.g1)), m.g2)
    if m.layer_id == 0:
        v_first = v
        k2, z, b, k2_b = kva(k, None, None, None, al, m.k_k, m.k_a, m.a0, None, True)
        k2_b = k2_b if GRAD_ALIAS else k2
        v2 = v2_b = v
    else:
        vl = mm(mm(xv_b, m.v1), m.v2)
        if VF_CHAIN and torch.is_grad_enabled():
            k2, v2, z, b, k2_b, v2_b, v_first = kva(k, v, v_first, vl, al, m.k_k, m.k_a, m.a0, m.v0, True, True)    # v_first: alias for the next layer
        else:
            k2, v2, z, b, k2_b, v2_b = kva(k, v, v_first, vl, al, m.k_k, m.k_a, m.a0, m.v0, True)
        if not GRAD_ALIAS:
            k2_b, v2_b = k2, v2
    s_end = None
    if want_state:
        if layout is not None:
            raise NotImplementedError("a carried state together with packed rows")
        if state0 is None:
            state0 = m.wkv_initial_state()
        if state0 is None:
            state0 = torch.zeros(r.shape[0], r.shape[2] // 64, 64, 64, dtype=torch.float32, device=r.device)
        y, s_end = RUN_CUDA_RWKV7g_state(r, w, k2, v2, z, b, state0, recompute_state=recompute_state)
    elif layout is not None:
        if getattr(m, "time_state", None) is not None:
            raise NotImplementedError("packed rows together with a tuned state: every segment would have to start from it")
        y = RUN_CUDA_RWKV7g_packed(r, w, k2, v2, z, b, layout, recompute_state=recompute_state)
    elif getattr(m, "time_state", None) is not None:      # state tuning: the recurrence starts from the layer's learnable state
        y, _ = RUN_CUDA_RWKV7g_state(r, w, k2, v2, z, b, m.wkv_initial_state(), recompute_state=recompute_state)
    else:
        y = RUN_CUDA_RWKV7g(r, w, k2, v2, z, b, recompute_state=recompute_state)
    y = post(y, r, k2_b, v2_b, g, m.ln_x.weight, m.ln_x.bias, m.r_k, m.ln_x.eps)
    if want_state:
        return linear(m.output, y), v_first, s_end
    return linear(m.output, y), v_first


def mix_prev(x, x_prev, *mus):
    """Inference-only `mix` whose shift sees `x_prev` (B,C) before the first token instead of zeros (stateful decode)."""
    B, T, C = x.shape
    x = x.contiguous()
    x_prev = x_prev.contiguous()
    mus_c = [m.reshape(C).contiguous() for m in mus]
    _chk(x, x_prev, *mus_c)
    outs = [torch.empty_like(x) for _ in mus]
    _glue("vrwkv_mix_fwd_prev_bf16", B * T, T, C, len(mus), x, x_prev, mus_c, outs, like=x)
    return tuple(outs)


@torch.no_grad()
def tmix_forward_stateful(m, x, v_first, state):
    """`tmix_forward` continuing from `state` (an RWKV7State): fused glue kernels, WKV through state.wkv."""
    lid = m.layer_id
    xr, xw, xk, xv, xa, xg = mix_prev(x, state.att_x[lid], m.x_r, m.x_w, m.x_k, m.x_v, m.x_a, m.x_g)
    state.att_x[lid].copy_(x[:, -1])
    r = m.receptance(xr)
    w = decay(torch.tanh(xw @ m.w1) @ m.w2, m.w0)
    k = m.key(xk)
    v = m.value(xv)
    al = (xa @ m.a1) @ m.a2
    g = torch.sigmoid(xg @ m.g1) @ m.g2
    if lid == 0:
        v_first = v
        k2, z, b = kva(k, None, None, None, al, m.k_k, m.k_a, m.a0, None)
        v2 = v
    else:
        vl = (xv @ m.v1) @ m.v2
        k2, v2, z, b = kva(k, v, v_first, vl, al, m.k_k, m.k_a, m.a0, m.v0)
    y = state.wkv(lid, r, w, k2, v2, z, b)
    y = post(y, r, k2, v2, g, m.ln_x.weight, m.ln_x.bias, m.r_k, m.ln_x.eps)
    return m.output(y), v_first


@torch.no_grad()
def cmix_forward_stateful(m, x, state):
    lid = m.layer_id
    (k,) = mix_prev(x, state.ffn_x[lid], m.x_k)
    state.ffn_x[lid].copy_(x[:, -1])
    return m.value(relu_sq(m.key(k)))


def cmix_forward(m, x):
    """RWKV_CMix_x070.forward (src/model.py:221-227)."""
    (k,) = mix(x, m.x_k)
    return cmix_from_mixed(m, k)


def cmix_from_mixed(m, k, recompute_relusq=False):
    h = linear(m.key, k)
    if (recompute_relusq and DGRAD_TN and m.value.bias is None and h.is_cuda and h.dtype == torch.bfloat16 and torch.is_grad_enabled()
            and h.requires_grad):
        return _ReluSqLinear.apply(h, m.value.weight)
    return linear(m.value, relu_sq(h))


# ---------------------------------------------------------------------------------------------------------------
# Image side (csrc/visual_ops.hip, vrwkv_ln_scatter_* in csrc/ln_fused.hip): pooling, context gate, ln_v + scatter
# (VisualRWKV-v7/v7.00/src/model.py:328-338,442-447,485-493)
# ---------------------------------------------------------------------------------------------------------------
def visual_supported(x):
    return x.is_cuda and x.dtype == torch.bfloat16 and x.shape[-1] % 8 == 0


def adaptive_pool(image_features, side_out):
    """nn.AdaptiveAvgPool2d(side_out) on token-major ViT features (B, L, D) -> (B, side_out^2, D) without the
    (B, D, H, W) permutes of VisualRWKV.adaptive_pooling; forward only (the towers are frozen and detached)."""
    x = image_features.detach().contiguous()
    _chk(x)
    B, Ln, D = x.shape
    side = int(round(Ln ** 0.5))
    if side * side != Ln:
        raise ValueError(f"{Ln} patch tokens are not a square grid")
    y = torch.empty(B, side_out * side_out, D, dtype=x.dtype, device=x.device)
    _glue("vrwkv_adaptive_pool_bf16", B, side, side_out, D, x, y, like=x)
    return y


class _Gate(torch.autograd.Function):
    """x * sigmoid(g) in one pass (model.py:337); backward dg (and dx when x needs it) in one pass."""

    @staticmethod
    def forward(ctx, x, g):
        x, g = x.contiguous(), g.contiguous()
        _chk(x, g)
        out = torch.empty_like(x)
        _glue("vrwkv_gate_fwd_bf16", x.numel(), x, g, out, like=x)
        ctx.save_for_backward(x, g)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, g = ctx.saved_tensors
        dout = dout.contiguous()
        dg = torch.empty_like(g)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        _glue("vrwkv_gate_bwd_bf16", x.numel(), x, g, dout, dg, dx, like=x)
        return dx, dg


def gate(x, g):
    return _Gate.apply(x, g)


def gelu_(x, tanh_approx=False):
    """nn.GELU of the frozen towers' MLPs, IN PLACE on a contiguous bf16 device tensor without autograd (timm Mlp through src/vision.py:123-134,
    src/sam.py MLPBlock): csrc/visual_ops.hip, 16 VALU operations per element where the eager erf kernel is VALU-bound at 2.3 TB/s."""
    _chk(x)
    if x.requires_grad or x.numel() % 8 != 0 or not x.is_contiguous():
        raise ValueError("gelu_: contiguous, no autograd, a multiple of 8 elements")
    _glue("vrwkv_gelu_bf16", x.numel(), x, x, 1 if tanh_approx else 0, like=x)
    return x


class _LnScatter(torch.autograd.Function):
    """embeds[row_index[n]] = LayerNorm(y[n]): ln_v of the projector fused with the masked scatter into the token
    embeddings (model.py:338 + :485-493).  `embeds` (rows, C) is modified in place and returned."""

    @staticmethod
    def forward(ctx, embeds, y, w, b, row_index, eps):
        y = y.contiguous()
        _chk(embeds, y, w, b)
        n, C = y.shape
        mean = torch.empty(n, dtype=torch.float32, device=y.device)
        rstd = torch.empty_like(mean)
        _glue("vrwkv_ln_scatter_fwd_bf16", n, C, float(eps), y, w, b, row_index, embeds, mean, rstd, like=y)
        ctx.mark_dirty(embeds)
        ctx.save_for_backward(y, w, mean, rstd, row_index)
        return embeds

    @staticmethod
    def backward(ctx, dout):
        y, w, mean, rstd, row_index = ctx.saved_tensors
        dout = dout.contiguous()
        n, C = y.shape
        dy = torch.empty_like(y)
        dwb = torch.empty(2, C, dtype=torch.float32, device=y.device)
        ws = torch.empty(hip_lib.load().vrwkv_add_ln_ws_floats(n, C), dtype=torch.float32, device=y.device)
        _glue("vrwkv_ln_gather_bwd_bf16", n, C, dout, row_index, y, mean, rstd, w, dy, dwb, ws, like=y)
        d_emb = None
        if ctx.needs_input_grad[0]:                    # rows that were overwritten do not reach the embedding
            R = dout.shape[0]                          # dropped features carry row -1: they zero a scratch row past the end
            d_emb = torch.empty(R + 1, C, dtype=dout.dtype, device=dout.device)
            d_emb[:R] = dout
            d_emb.index_fill_(0, torch.where(row_index < 0, R, row_index), 0)
            d_emb = d_emb[:R]
        return d_emb, dy, dwb[0].to(w.dtype), dwb[1].to(w.dtype), None, None


def ln_scatter(embeds2d, y2d, ln, row_index):
    return _LnScatter.apply(embeds2d, y2d, ln.weight, ln.bias, row_index, ln.eps)


# ------------------------------------------------------------------------------------------------
# Visual token compressor (VisualRWKV-v7/v7.04 src/model.py:327-374,516-529): time reversal around every second Block, and the tail
# ln_out + unpad + AdaptiveAvgPool1d over tokens + scatter (csrc/fused_ops.hip: flip_add; csrc/ln_fused.hip: ln_pool_*)
# ------------------------------------------------------------------------------------------------
class _FlipAdd(torch.autograd.Function):
    """out[b, T-1-t] = x[b, t] + delta[b, t] (delta may be None: the pure flip).  Its own backward: d x = d delta = flip(d out), one tensor."""

    @staticmethod
    def forward(ctx, x, delta):
        B, T, C = x.shape
        x = x.contiguous()
        delta = delta.contiguous() if delta is not None else None
        _chk(x, delta)
        if delta is not None and delta.shape != x.shape:
            raise ValueError("flip_add: x and delta must have the same shape")
        out = torch.empty_like(x)
        _glue("vrwkv_flip_add_bf16", B, T, C, x, delta, out, like=x)
        ctx.has_delta = delta is not None
        return out

    @staticmethod
    def backward(ctx, dout):
        B, T, C = dout.shape
        dout = dout.contiguous()
        _chk(dout)
        dx = torch.empty_like(dout)
        _glue("vrwkv_flip_add_bf16", B, T, C, dout, None, dx, like=dout)
        return dx, (dx if ctx.has_delta else None)


def flip_add(x, delta=None):
    """(x + delta).flip(1) of (B, T, C) bf16 in one pass; delta may be None."""
    return _FlipAdd.apply(x, delta)


class _LnPoolScatter(torch.autograd.Function):
    """The compressor's tail: LayerNorm(x + delta) of (B, T, C), the first `pad` rows of every sample dropped, AdaptiveAvgPool1d(Lout) over the
    remaining tokens, output b * Lout + i written to row row_index[b * Lout + i] of `embeds` (rows, C), which is modified in place and returned; a
    negative row drops that output.  embeds = None: a new dense (B * Lout, C) tensor in order (row_index must be None too)."""

    @staticmethod
    def forward(ctx, embeds, x, delta, w, b, row_index, pad, Lout, eps):
        B, T, C = x.shape
        x = x.contiguous()
        delta = delta.contiguous() if delta is not None else None
        wc, bc = w.contiguous(), b.contiguous()
        _chk(embeds, x, delta, wc, bc)
        if (embeds is None) != (row_index is None):
            raise ValueError("ln_pool_scatter: `embeds` and `row_index` go together")
        if row_index is not None and (row_index.dtype != torch.int64 or row_index.numel() != B * Lout or row_index.device != x.device
                                      or not row_index.is_contiguous()):
            raise ValueError(f"ln_pool_scatter: row_index must hold {B * Lout} contiguous int64 rows on {x.device}")
        if embeds is not None and (embeds.dim() != 2 or embeds.shape[1] != C or not embeds.is_contiguous()):
            raise ValueError("ln_pool_scatter: embeds must be a contiguous (rows, C) tensor")
        out = embeds if embeds is not None else torch.empty(B * Lout, C, dtype=x.dtype, device=x.device)
        xn = torch.empty_like(x) if delta is not None else x
        mean = torch.empty(B * T, dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        _glue("vrwkv_ln_pool_scatter_fwd_bf16", B, T, int(pad), int(Lout), C, float(eps), x, delta, wc, bc, row_index, xn if delta is not None else None,
              out, mean, rstd, like=x)
        if embeds is not None:
            ctx.mark_dirty(embeds)
        ctx.save_for_backward(xn, mean, rstd, wc, row_index)
        ctx.geom = (int(pad), int(Lout))
        ctx.has_delta, ctx.scatter = delta is not None, embeds is not None
        return out

    @staticmethod
    def backward(ctx, dout):
        xn, mean, rstd, wc, row_index = ctx.saved_tensors
        B, T, C = xn.shape
        pad, Lout = ctx.geom
        dout = dout.contiguous()
        _chk(dout)
        dx = torch.empty_like(xn)
        dwb = torch.empty(2, C, dtype=torch.float32, device=xn.device)
        ws = torch.empty(hip_lib.load().vrwkv_add_ln_ws_floats(B * T, C), dtype=torch.float32, device=xn.device)
        _glue("vrwkv_ln_pool_gather_bwd_bf16", B, T, pad, Lout, C, dout, row_index, xn, mean, rstd, wc, dx, dwb, ws, like=xn)
        d_emb = None
        if ctx.scatter and ctx.needs_input_grad[0]:    # as _LnScatter: rows that were overwritten do not reach the embedding
            R = dout.shape[0]
            d_emb = torch.empty(R + 1, C, dtype=dout.dtype, device=dout.device)
            d_emb[:R] = dout
            d_emb.index_fill_(0, torch.where(row_index < 0, R, row_index), 0)
            d_emb = d_emb[:R]
        return d_emb, dx, (dx if ctx.has_delta else None), dwb[0].to(wc.dtype), dwb[1].to(wc.dtype), None, None, None, None


def ln_pool_scatter(x, delta, ln, pad, Lout, embeds2d=None, row_index=None):
    """See `_LnPoolScatter`; returns embeds2d (modified in place), or the dense (B * Lout, C) result when it is None."""
    return _LnPoolScatter.apply(embeds2d, x, delta, ln.weight, ln.bias, row_index, pad, Lout, ln.eps)


VTC_TAIL = os.environ.get("VRWKV_VTC_TAIL", "1") != "0"           # A/B switch: 0 = add_ln, torch's adaptive_avg_pool1d and index_copy for the tail


def vtc_supported(vtc, x):
    """May the compressor take vtc_forward?  bf16 on the GPU with args.fused, rows the LayerNorm kernels accept."""
    return (bool(getattr(vtc.args, "fused", False)) and add_ln_supported(x) and x.dim() == 3 and vtc.ln_out.weight.dtype == torch.bfloat16
            and len(vtc.blocks) > 0)


def vtc_pad(x):
    """VisualTokenCompressor.pad_left (src/model.py:334-342, 353-356): ZERO rows on the left up to a multiple of 16 tokens.  Returns (x, pad)."""
    pad = (-x.shape[1]) % 16
    if pad:
        x = torch.cat((torch.zeros(x.shape[0], pad, x.shape[2], dtype=x.dtype, device=x.device), x), dim=1)
    return x, pad


def vtc_forward(vtc, x, grad_cp=0, layout=None):
    """The Blocks of a rwkv7.VisualTokenCompressor on the already padded (B, T, C) rows (VisualTokenCompressor.forward, src/model.py:358-370), through
    _block_segment on the (x, pending delta) residual stream: every second Block runs on the time-reversed rows.  The flip into a reversed Block takes
    the pending residual add with it (flip_add), and so does the flip out of it, so neither add is paid twice.  v_first is written by Block 0 alone
    and only read after it: it is flipped once, every reversed Block reads that copy, and its gradient comes back through that one flip.
    The pad rows are ordinary rows, as in the reference: after a reversed Block they hold what the recurrence left there.
    grad_cp as in blocks_forward; mode 1 checkpoints the Block, the flips stay outside.  Returns (x, delta): ln_out is the caller's (ln_pool_scatter,
    or add_ln for the 'step' reduction)."""
    if layout is not None:
        raise NotImplementedError("packed rows inside the compressor: the flips reverse whole rows (rwkv7.VisualTokenCompressor.forward)")
    grad_cp = int(grad_cp) if torch.is_grad_enabled() else 0
    if grad_cp not in (0, 1, 2):
        raise ValueError(f"grad_cp = {grad_cp}: 0, 1 or 2 (see blocks_forward)")
    if x.shape[1] % 16 != 0:
        raise ValueError(f"vtc_forward: T = {x.shape[1]} must be a multiple of 16 (vtc_pad)")
    x = vtc.blocks[0].ln0(x)
    v_fwd, v_rev = torch.empty_like(x), None
    delta = None
    for i, block in enumerate(vtc.blocks):
        rev = i % 2 == 1
        if rev:
            x, delta = flip_add(x, delta), None
            if v_rev is None:
                v_rev = flip_add(v_fwd)
        v_in = v_rev if rev else v_fwd
        if grad_cp == 1:
            from torch.utils.checkpoint import checkpoint
            x, delta, v_out = checkpoint(_block_segment, block, x, delta, v_in, False, None, None, None, use_reentrant=False)
        else:
            x, delta, v_out = _block_segment(block, x, delta, v_in, grad_cp == 2)
        if i > 0 and (v_out.data_ptr() != v_in.data_ptr() or v_out.shape != v_in.shape):
            raise AssertionError(f"vtc_forward: Block {i} returned another v_first than it was given; the flipped copy cannot be reused")
        if rev:
            v_rev = v_out
            x, delta = flip_add(x, delta), None
        else:
            v_fwd = v_out
    return x, delta


def vtc_compress(vtc, feats, Lout, reduction="pool", embeds2d=None, row_index=None, grad_cp=0):
    """compress_visual_tokens on the fused path (src/model.py:516-529): feats (B, N L, C) -> pad -> Blocks -> ln_out -> unpad -> reduction.
    'pool': AdaptiveAvgPool1d(Lout) over tokens, written into rows `row_index` of embeds2d (returned), or returned as (B, Lout, C) when embeds2d is None.
    'step': every (N L // Lout)-th token, as the reference's slice; (B, ceil(N L / step), C)."""
    B, Lin, C = feats.shape
    x, pad = vtc_pad(feats)
    x, delta = vtc_forward(vtc, x, grad_cp)
    if reduction == "step":
        _, h = add_ln(x, delta, vtc.ln_out)
        return h[:, pad:][:, ::Lin // Lout]
    if reduction != "pool":
        raise ValueError(f"reduction = {reduction!r}: 'pool' or 'step'")
    if not VTC_TAIL:                                # the composite of what existed before the tail kernels
        _, h = add_ln(x, delta, vtc.ln_out)
        pooled = F.adaptive_avg_pool1d(h[:, pad:].permute(0, 2, 1), Lout).permute(0, 2, 1)
        if embeds2d is None:
            return pooled
        keep = row_index >= 0
        return embeds2d.index_copy(0, row_index[keep], pooled.reshape(B * Lout, C)[keep])
    out = ln_pool_scatter(x, delta, vtc.ln_out, pad, Lout, embeds2d, row_index)
    return out if embeds2d is not None else out.view(B, Lout, C)


# ------------------------------------------------------------------------------------------------
# Patch embedding of the frozen towers (csrc/patch_embed_kernels.h)
# ------------------------------------------------------------------------------------------------
_PATCH_SIZES = (14, 16)


def patch_embed_supported(x, patch, dim):
    if not (visual_supported(x) and x.dim() == 4 and x.shape[1] == 3 and patch in _PATCH_SIZES and dim % 32 == 0):
        return False
    H, W = x.shape[-2:]
    return H % patch == 0 and W % patch == 0 and ((H // patch) * (W // patch)) % 64 == 0


def padded_patch_weight(weight):
    """(N, 3, p, p) conv weight -> (N, KP) bf16 with zero columns up to the MFMA K multiple the kernel reads."""
    N = weight.shape[0]
    K = weight[0].numel()
    KP = hip_lib.load().vrwkv_patch_embed_kp(int(weight.shape[-1]))
    wp = torch.zeros(N, KP, dtype=torch.bfloat16, device=weight.device)
    wp[:, :K] = weight.detach().reshape(N, K)
    return wp


def cached_padded_patch_weight(module, weight):
    """The padded weight kept on the module that owns `weight` (frozen towers: built once); rebuilt when the parameter
    is modified in place, replaced, or an optimizer step bumps the process-wide parameter generation."""
    from . import param_state
    # the optimizer generation only matters for trainable weights (it is bumped every step; the frozen towers' weights are
    # not in the ZeRO flat buffer and data_ptr / _version / shape identify them)
    gen = param_state.generation() if weight.requires_grad else -1
    key = (weight.data_ptr(), weight._version, gen, tuple(weight.shape), weight.device)
    hit = getattr(module, "_padded_patch_weight", None)
    if hit is None or hit[0] != key:
        hit = (key, padded_patch_weight(weight))
        module._padded_patch_weight = hit
    return hit[1]


def patch_embed(x, weight, bias, pos=None, prefix=None, padded_weight=None):
    """out[:, P:, :] = conv2d(x, weight, bias, stride=patch).flatten(2).T + pos; out[:, :P] = prefix tokens.
    x (B,3,H,W) bf16; weight (N,3,p,p); bias (N) or None; pos (M,N) or None; prefix (P,N) or None (class / register
    tokens, copied as they are).  Forward only (the towers are frozen, src/model.py:349,368)."""
    B, _, H, W = x.shape
    N, patch = weight.shape[0], weight.shape[-1]
    M = (H // patch) * (W // patch)
    npre = 0 if prefix is None else prefix.shape[0]
    x = x.contiguous()
    out = torch.empty(B, npre + M, N, dtype=torch.bfloat16, device=x.device)
    if npre:
        out[:, :npre] = prefix.to(torch.bfloat16)
    wp = padded_weight if padded_weight is not None else padded_patch_weight(weight)
    bias = None if bias is None else bias.detach().to(torch.bfloat16).contiguous()
    pos = None if pos is None else pos.detach().to(torch.bfloat16).reshape(M, N).contiguous()
    _glue("vrwkv_patch_embed_bf16", B, H, W, patch, N, x, wp, bias, pos, out, npre + M, npre, like=x)
    return out


# ------------------------------------------------------------------------------------------------
# The trainable RWKV vision encoder of VisualRWKV-v7/v7.10 (src/model.py:367-415: VRWKV): patch embedding with a weight gradient
# (csrc/patch_wgrad.h), plain Blocks, and the tail ln_out + scatter + mean over tokens (csrc/ln_kernels.h: ln_scatter_mean_*)
# ------------------------------------------------------------------------------------------------
PATCH_WGRAD = os.environ.get("VRWKV_PATCH_WGRAD", "1") != "0"     # A/B switch: 0 = F.unfold + the library's GEMM for the weight gradient
VRWKV_TAIL = os.environ.get("VRWKV_TAIL", "1") != "0"             # A/B switch: 0 = add_ln, index_copy and mean for the tail


def patch_wgrad_supported(x, weight):
    """May the weight gradient of a patch embedding run as vrwkv_patch_embed_wgrad_bf16?  P = 16 (P = 14: 28-byte pixel segments cannot be moved by
    LDS-DMA), N % 256 == 0, B Mimg % 32 == 0, images below 4 GiB."""
    if not (visual_supported(x) and x.dim() == 4 and x.shape[1] == 3 and weight.dim() == 4 and weight.dtype == torch.bfloat16):
        return False
    B, _, H, W = x.shape
    N, patch = weight.shape[0], weight.shape[-1]
    return hip_lib.load().vrwkv_patch_embed_wgrad_ws_floats(B, H, W, patch, N) > 0


class _PatchEmbedTrain(torch.autograd.Function):
    """conv2d(x, weight, bias, stride=patch).flatten(2).transpose(1, 2) with a trained weight: the forward is patch_embed's kernel (for P = 16 the
    weight viewed as (N, 768) is already what it reads: no copy), the backward vrwkv_patch_embed_wgrad_bf16 straight from the pixels -- or, for
    shapes that kernel refuses (P = 14, N % 256 != 0), F.unfold and a GEMM.  There is no pixel gradient."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        if x.requires_grad:
            raise ValueError("patch_embed_train: no gradient flows to the pixels")
        N, patch = weight.shape[0], weight.shape[-1]
        x = x.contiguous()
        wc = weight.contiguous()
        K = wc[0].numel()
        wp = wc.view(N, K) if hip_lib.load().vrwkv_patch_embed_kp(patch) == K else padded_patch_weight(wc)
        out = patch_embed(x, wc, bias, None, None, padded_weight=wp)
        ctx.save_for_backward(x)
        ctx.wshape, ctx.has_bias, ctx.kernel = tuple(weight.shape), bias is not None, PATCH_WGRAD and patch_wgrad_supported(x, wc)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, = ctx.saved_tensors
        B, _, H, W = x.shape
        N, _, patch, _ = ctx.wshape
        d2 = dout.contiguous().view(-1, N)
        if not ctx.kernel:
            cols = F.unfold(x, patch, stride=patch).transpose(1, 2).reshape(d2.shape[0], -1)
            dw = wgrad_big(d2, cols) if wgrad_big_supported(d2, cols) else d2.t() @ cols
            return None, dw.view(ctx.wshape), (d2.sum(0, dtype=torch.float32).to(d2.dtype) if ctx.has_bias else None)
        dw = torch.empty(ctx.wshape, dtype=torch.bfloat16, device=x.device)
        db = torch.empty(N, dtype=torch.bfloat16, device=x.device) if ctx.has_bias else None
        ws = torch.empty(hip_lib.load().vrwkv_patch_embed_wgrad_ws_floats(B, H, W, patch, N), dtype=torch.float32, device=x.device)
        _glue("vrwkv_patch_embed_wgrad_bf16", B, H, W, patch, N, x, d2, dw, db, ws, like=x)
        return None, dw, db


def patch_embed_train(x, weight, bias):
    """See `_PatchEmbedTrain`: (B, 3, H, W) bf16 pixels -> (B, tokens, N) with gradients for weight and bias."""
    return _PatchEmbedTrain.apply(x, weight, bias)


class _LnScatterMean(torch.autograd.Function):
    """VRWKV's tail: LayerNorm(x + delta) of (B, L, C); row b L + t is written to row row_index[b L + t] of `embeds` (rows, C), which is modified in
    place and returned (a negative row is dropped), and pooled (B, C) = the mean over tokens of the same normalised rows (dropped rows included).
    embeds = None: a new dense (B L, C) tensor in order (row_index must be None too).  embeds must not be a view of another tensor: autograd
    refuses an op with two outputs that writes into one."""

    @staticmethod
    def forward(ctx, embeds, x, delta, w, b, row_index, eps):
        B, L, C = x.shape
        x = x.contiguous()
        delta = delta.contiguous() if delta is not None else None
        wc, bc = w.contiguous(), b.contiguous()
        _chk(embeds, x, delta, wc, bc)
        if (embeds is None) != (row_index is None):
            raise ValueError("ln_scatter_mean: `embeds` and `row_index` go together")
        if row_index is not None and (row_index.dtype != torch.int64 or row_index.numel() != B * L or row_index.device != x.device
                                      or not row_index.is_contiguous()):
            raise ValueError(f"ln_scatter_mean: row_index must hold {B * L} contiguous int64 rows on {x.device}")
        if embeds is not None and (embeds.dim() != 2 or embeds.shape[1] != C or not embeds.is_contiguous()):
            raise ValueError("ln_scatter_mean: embeds must be a contiguous (rows, C) tensor")
        out = embeds if embeds is not None else torch.empty(B * L, C, dtype=x.dtype, device=x.device)
        pooled = torch.empty(B, C, dtype=x.dtype, device=x.device)
        xn = torch.empty_like(x) if delta is not None else x
        mean = torch.empty(B * L, dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        ws = torch.empty(hip_lib.load().vrwkv_ln_scatter_mean_ws_floats(B, L, C), dtype=torch.float32, device=x.device)
        _glue("vrwkv_ln_scatter_mean_fwd_bf16", B, L, C, float(eps), x, delta, wc, bc, row_index, xn if delta is not None else None, out, pooled, mean,
              rstd, ws, like=x)
        if embeds is not None:
            ctx.mark_dirty(embeds)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(xn, mean, rstd, wc, row_index)
        ctx.has_delta, ctx.scatter = delta is not None, embeds is not None
        return out, pooled

    @staticmethod
    def backward(ctx, dout, dpooled):
        xn, mean, rstd, wc, row_index = ctx.saved_tensors
        B, L, C = xn.shape
        if dout is None and dpooled is None:
            return (None,) * 7
        dout = dout.contiguous() if dout is not None else None
        dpooled = dpooled.contiguous() if dpooled is not None else None
        _chk(dout, dpooled)
        dx = torch.empty_like(xn)
        dwb = torch.empty(2, C, dtype=torch.float32, device=xn.device)
        ws = torch.empty(hip_lib.load().vrwkv_ln_scatter_mean_ws_floats(B, L, C), dtype=torch.float32, device=xn.device)
        _glue("vrwkv_ln_gather_mean_bwd_bf16", B, L, C, dout, row_index, dpooled, xn, mean, rstd, wc, dx, dwb, ws, like=xn)
        d_emb = None
        if ctx.scatter and ctx.needs_input_grad[0] and dout is not None:    # as _LnScatter: rows that were overwritten do not reach the embedding
            R = dout.shape[0]
            d_emb = torch.empty(R + 1, C, dtype=dout.dtype, device=dout.device)
            d_emb[:R] = dout
            d_emb.index_fill_(0, torch.where(row_index < 0, R, row_index), 0)
            d_emb = d_emb[:R]
        return d_emb, dx, (dx if ctx.has_delta else None), dwb[0].to(wc.dtype), dwb[1].to(wc.dtype), None, None


def ln_scatter_mean(x, delta, ln, embeds2d=None, row_index=None):
    """See `_LnScatterMean`; returns (embeds2d modified in place -- or the dense (B L, C) rows when it is None --, pooled (B, C))."""
    return _LnScatterMean.apply(embeds2d, x, delta, ln.weight, ln.bias, row_index, ln.eps)


def vrwkv_supported(vrwkv, images):
    """May a rwkv7.VRWKV take vrwkv_forward?  bf16 pixels on the GPU with args.fused, a patch embedding the forward kernel accepts, rows the
    LayerNorm kernels accept."""
    w = vrwkv.emb.weight
    return (bool(getattr(vrwkv.args, "fused", False)) and images.dim() == 4 and w.dtype == torch.bfloat16 and vrwkv.ln_out.weight.dtype == torch.bfloat16
            and patch_embed_supported(images, w.shape[-1], w.shape[0]) and w.shape[0] % 64 == 0 and w.shape[0] <= 8192 and len(vrwkv.blocks) > 0)


def vrwkv_forward(vrwkv, images, embeds2d=None, row_index=None, grad_cp=0):
    """rwkv7.VRWKV.forward on the fused path (src/model.py:376-395): patch embedding -> Blocks on the (x, pending delta) stream -> the tail kernel,
    which applies ln_out to every token, writes it into rows `row_index` of embeds2d (or a dense (B, L, C) tensor) and forms the mean over tokens
    for the ImageNet head.  Returns (embeds2d modified in place, or the features (B, L, C); logits (B, 1000))."""
    x = patch_embed_train(images, vrwkv.emb.weight, vrwkv.emb.bias)
    B, L, C = x.shape
    if L % 16 != 0:
        raise ValueError(f"vrwkv_forward: {L} tokens per image must be a multiple of 16")
    x, delta, _ = _blocks_walk(vrwkv, x, grad_cp)
    if not VRWKV_TAIL:                              # the composite of what existed before the tail kernels
        _, h = add_ln(x, delta, vrwkv.ln_out)
        logits = vrwkv.head(h.mean(dim=1))
        if embeds2d is None:
            return h, logits
        keep = row_index >= 0
        return embeds2d.index_copy(0, row_index[keep], h.reshape(B * L, C)[keep]), logits
    out, pooled = ln_scatter_mean(x, delta, vrwkv.ln_out, embeds2d, row_index)
    return (out if embeds2d is not None else out.view(B, L, C)), vrwkv.head(pooled)
