"""RWKV-7 ("x070") language-model blocks on top of the gfx950 WKV7 operator.

Host-side mirror of the reference's operator/module surface for the hot path
(VisualRWKV-v7/v7.00/src/model.py:76-325): same class names, constructor arguments, forward
signatures, parameter names (=> identical state-dict keys) and the same arithmetic, so that a
checkpoint of the reference loads unchanged and the v7.00 trainer/evaluator can call these classes
in place of its own.  What differs is underneath: the WKV7 recurrence is the chunked MFMA kernel of
libvisualrwkv_hip.so, and the element-wise glue around it can run as fused HIP kernels
(`visualrwkv_amd.fused`, opt-in per module through `fused=True`).
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn
from torch.nn import functional as F

from .wkv7 import CHUNK_LEN, RUN_CUDA_RWKV7g, RUN_CUDA_RWKV7g_packed, RUN_CUDA_RWKV7g_state

STOP_TOKEN_INDEX = 261        # src/dataset.py:20  ("\n\n"), used to left-pad to a multiple of CHUNK_LEN
IGNORE_INDEX = -100           # src/dataset.py:17
IMAGE_TOKEN_INDEX = 65535     # src/dataset.py:18


def _lora_rank(C: int, factor: float, power: float = 0.5) -> int:
    """max(32, round(factor * C**power / 32) * 32)   (src/model.py:118,127,133,140)"""
    return max(32, int(round((factor * (C ** power)) / 32) * 32))


def _ortho(rows: int, cols: int, scale: float) -> torch.Tensor:
    w = torch.zeros(rows, cols)
    gain = math.sqrt(rows / cols) if rows > cols else 1.0
    nn.init.orthogonal_(w, gain=gain * scale)
    return w


def time_shift(x: torch.Tensor, layout=None, prev=None) -> torch.Tensor:
    """x_{t-1} with zeros at t = 0 of every sample (nn.ZeroPad2d((0,0,1,-1)), src/model.py:149).  With a wkv7.PackedLayout the first token
    of every segment of a packed row reads zeros too, and no gradient goes from it to the token before.  prev (B, C): the token before the
    first one (a row cut into segments, TrainCarry) in place of the zeros; gradients flow into it."""
    if prev is not None:
        if layout is not None:
            raise NotImplementedError("time_shift: a carried token together with packed rows")
        return torch.cat((prev.to(x.dtype).unsqueeze(1), x[:, :-1]), dim=1)
    xs = F.pad(x, (0, 0, 1, -1))
    if layout is not None:
        xs = xs.masked_fill(layout.first.view(x.shape[0], x.shape[1], 1).bool(), 0)
    return xs


class TrainCarry:
    """What crosses a cut when a long row is trained in segments (VisualRWKV.train_step_cut; not in the reference, whose training op has no
    state).  Per layer: `att_x` / `ffn_x` (B, C) = the ln1 / ln2 output of the last token before the cut, which the time-mix / channel-mix
    shift of the next segment reads, and `S` (B, H, 64, 64) fp32 (fp64 for an fp64 model) = the WKV state.  Unlike the inference RWKV7State
    these are ordinary autograd tensors: the modules RETURN the next carry instead of updating one in place, and gradients flow through
    all three.  An entry of None is the start of a row: the shift reads zeros and the state starts from zeros, or from the layer's
    `time_state` under args.state_tune."""

    def __init__(self, n_layer, layers=None):
        self.layers = list(layers) if layers is not None else [(None, None, None)] * n_layer
        if len(self.layers) != n_layer:
            raise ValueError(f"TrainCarry: {len(self.layers)} layers given for a model of {n_layer}")

    def __getitem__(self, i):
        return self.layers[i]

    def tensors(self):
        """Every tensor of the carry, layer by layer (att_x, ffn_x, S); None entries are left out."""
        return [t for layer in self.layers for t in layer if t is not None]

    def detach(self, requires_grad=False):
        """The same values cut from their graph (as leaves that collect a gradient with requires_grad)."""
        leaf = lambda t: None if t is None else t.detach().requires_grad_(requires_grad)
        return TrainCarry(len(self.layers), [tuple(leaf(t) for t in layer) for layer in self.layers])


def _carry_state0(m, carry_S, B, like):
    """The state a segment's WKV recurrence starts from: the carried one, else the layer's tuned state, else zeros."""
    if carry_S is not None:
        return carry_S
    s0 = m.wkv_initial_state()
    if s0 is not None:
        return s0
    return torch.zeros(B, m.n_head, m.head_size, m.head_size, device=like.device,
                       dtype=torch.float64 if like.dtype == torch.float64 else torch.float32)


class RWKV_Tmix_x070(nn.Module):
    """Time-mix of RWKV-7 (src/model.py:76-195)."""

    def __init__(self, args, layer_id):
        super().__init__()
        self.args = args
        self.layer_id = layer_id
        self.head_size = args.head_size_a
        self.n_head = args.dim_att // self.head_size
        assert args.dim_att % self.n_head == 0
        H, N, C = self.n_head, self.head_size, args.n_embd

        with torch.no_grad():
            r01 = layer_id / (args.n_layer - 1) if args.n_layer > 1 else 0.0   # 0 -> 1 over depth
            r10 = 1.0 - (layer_id / args.n_layer)                                # 1 -> ~0
            ddd = (torch.arange(C, dtype=torch.float32) / C).view(1, 1, C)
            self.x_r = nn.Parameter(1.0 - torch.pow(ddd, 0.2 * r10))
            self.x_w = nn.Parameter(1.0 - torch.pow(ddd, 0.9 * r10))
            self.x_k = nn.Parameter(1.0 - (torch.pow(ddd, 0.9 * r10) + 0.4 * r01))
            self.x_v = nn.Parameter(1.0 - (torch.pow(ddd, 0.4 * r10) + 0.6 * r01))
            self.x_a = nn.Parameter(1.0 - torch.pow(ddd, 0.9 * r10))
            self.x_g = nn.Parameter(1.0 - torch.pow(ddd, 0.2 * r10))

            d_decay = _lora_rank(C, 1.8)
            self.w1 = nn.Parameter(torch.zeros(C, d_decay))
            self.w2 = nn.Parameter(_ortho(d_decay, C, 0.1))
            n = torch.arange(C, dtype=torch.float32)
            decay_speed = -7 + 5 * (n / (C - 1)) ** (0.85 + 1.0 * r01 ** 0.5)
            self.w0 = nn.Parameter(decay_speed.reshape(1, 1, C) + 0.5)          # +0.5: soft-clamp offset

            d_aaa = _lora_rank(C, 1.8)
            self.a1 = nn.Parameter(torch.zeros(C, d_aaa))
            self.a2 = nn.Parameter(_ortho(d_aaa, C, 0.1))
            self.a0 = nn.Parameter(torch.zeros(1, 1, C))

            d_mv = _lora_rank(C, 1.3)
            if layer_id != 0:                                                    # layer 0 defines v_first
                self.v1 = nn.Parameter(torch.zeros(C, d_mv))
                self.v2 = nn.Parameter(_ortho(d_mv, C, 0.1))
                self.v0 = nn.Parameter(torch.zeros(1, 1, C) + 1.0)

            d_gate = _lora_rank(C, 0.6, 0.8)
            self.g1 = nn.Parameter(torch.zeros(C, d_gate))
            self.g2 = nn.Parameter(_ortho(d_gate, C, 0.1))

            self.k_k = nn.Parameter(torch.ones(1, 1, C) * 0.85)
            self.k_a = nn.Parameter(torch.ones(1, 1, C))
            self.r_k = nn.Parameter(torch.zeros(H, N))

            self.receptance = nn.Linear(C, C, bias=False)
            self.key = nn.Linear(C, C, bias=False)
            self.value = nn.Linear(C, C, bias=False)
            self.output = nn.Linear(C, C, bias=False)
            self.ln_x = nn.GroupNorm(H, C, eps=(1e-5) * (args.head_size_divisor ** 2))   # eps = 64e-5

            self.receptance.weight.data.uniform_(-0.5 / (C ** 0.5), 0.5 / (C ** 0.5))
            self.key.weight.data.uniform_(-0.05 / (C ** 0.5), 0.05 / (C ** 0.5))
            self.value.weight.data.uniform_(-0.5 / (C ** 0.5), 0.5 / (C ** 0.5))
            self.output.weight.data.zero_()
            if getattr(args, "state_tune", 0):
                # state tuning (not in the reference): a learnable initial WKV state per head, [value row][key column] like every state of
                # this package.  An ordinary parameter of the model's dtype; the op receives it in fp32 (wkv_initial_state)
                self.time_state = nn.Parameter(torch.zeros(H, N, N))

    def wkv_initial_state(self):
        """The learnable initial WKV state (H,64,64) in the dtype the op takes (fp32; fp64 for an fp64 model), or None without state tuning."""
        ts = getattr(self, "time_state", None)
        if ts is None:
            return None
        return ts if ts.dtype == torch.float64 else ts.float()

    def forward(self, x, v_first, state=None, layout=None, carry=None):
        """`state` (an RWKV7State; inference: no gradient flows through it) carries the previous token and the WKV state across calls.
        `layout` (a wkv7.PackedLayout; training on packed rows): the shift and the WKV state restart at every segment.
        `carry` (training across a cut, TrainCarry): (att_x, S) entering this segment, either may be None; the call then returns
        (out, v_first, (att_x, S) leaving it), with gradients through both.  This is the PyTorch statement of the shift; the fused kernels
        take a carry through fused.blocks_forward."""
        B, T, C = x.size()
        H = self.n_head
        if carry is not None and (state is not None or layout is not None):
            raise NotImplementedError("a training carry together with an inference state or packed rows")
        if layout is not None and (state is not None or getattr(self, "time_state", None) is not None):
            raise NotImplementedError("packed rows together with a carried or tuned state: every segment would have to start from it")
        if getattr(self.args, "fused", False) and x.is_cuda and layout is None and carry is None:
            from . import fused
            if state is None:
                return fused.tmix_forward(self, x, v_first)
            if not torch.is_grad_enabled() and x.dtype == torch.bfloat16:
                return fused.tmix_forward_stateful(self, x, v_first, state)
        x_last = x[:, -1]
        if carry is not None:
            xx = time_shift(x, None, carry[0]) - x
        elif state is None:
            xx = time_shift(x, layout) - x
        else:
            xx = torch.cat((state.att_x[self.layer_id].unsqueeze(1), x[:, :-1]), dim=1) - x
            state.att_x[self.layer_id].copy_(x[:, -1])          # in place: the state tensors are stable addresses (HIP graphs)
        xr = x + xx * self.x_r
        xw = x + xx * self.x_w
        xk = x + xx * self.x_k
        xv = x + xx * self.x_v
        xa = x + xx * self.x_a
        xg = x + xx * self.x_g

        r = self.receptance(xr)
        w = -F.softplus(-(self.w0 + torch.tanh(xw @ self.w1) @ self.w2)) - 0.5   # w_raw <= -0.5
        k = self.key(xk)
        v = self.value(xv)
        if self.layer_id == 0:
            v_first = v
        else:
            v = v + (v_first - v) * torch.sigmoid(self.v0 + (xv @ self.v1) @ self.v2)
        a = torch.sigmoid(self.a0 + (xa @ self.a1) @ self.a2)
        g = torch.sigmoid(xg @ self.g1) @ self.g2

        kk = k * self.k_k
        kk = F.normalize(kk.view(B, T, H, -1), dim=-1, p=2.0).view(B, T, C)
        k = k * (1 + (a - 1) * self.k_a)

        s_end = None
        if carry is not None:
            x, s_end = RUN_CUDA_RWKV7g_state(r, w, k, v, -kk, kk * a, _carry_state0(self, carry[1], B, x))
        elif layout is not None:
            x = RUN_CUDA_RWKV7g_packed(r, w, k, v, -kk, kk * a, layout)
        elif state is None and getattr(self, "time_state", None) is not None:
            x, _ = RUN_CUDA_RWKV7g_state(r, w, k, v, -kk, kk * a, self.wkv_initial_state())
        elif state is None:
            x = RUN_CUDA_RWKV7g(r, w, k, v, -kk, kk * a)
        else:
            x = state.wkv(self.layer_id, r, w, k, v, -kk, kk * a)
        x = self.ln_x(x.view(B * T, C)).view(B, T, C)
        x = x + ((r.view(B, T, H, -1) * k.view(B, T, H, -1) * self.r_k).sum(dim=-1, keepdim=True)
                 * v.view(B, T, H, -1)).view(B, T, C)
        x = self.output(x * g)
        if carry is not None:
            return x, v_first, (x_last, s_end)
        return x, v_first


class RWKV_CMix_x070(nn.Module):
    """Channel-mix FFN of RWKV-7 (src/model.py:200-227): shift-lerp -> C->4C -> relu^2 -> 4C->C."""

    def __init__(self, args, layer_id):
        super().__init__()
        self.args = args
        self.layer_id = layer_id
        C = args.n_embd
        with torch.no_grad():
            r10 = 1.0 - (layer_id / args.n_layer)
            ddd = (torch.arange(C, dtype=torch.float32) / C).view(1, 1, C)
            self.x_k = nn.Parameter(1.0 - torch.pow(ddd, r10 ** 4))
        self.key = nn.Linear(C, C * 4, bias=False)
        self.value = nn.Linear(C * 4, C, bias=False)
        self.key.weight.data.uniform_(-0.5 / (C ** 0.5), 0.5 / (C ** 0.5))
        self.value.weight.data.zero_()

    def forward(self, x, state=None, layout=None, carry=None):
        """carry (training across a cut): a 1-tuple (ffn_x,) entering this segment (ffn_x may be None); returns (out, ffn_x leaving it)."""
        if carry is not None and (state is not None or layout is not None):
            raise NotImplementedError("a training carry together with an inference state or packed rows")
        if getattr(self.args, "fused", False) and x.is_cuda and layout is None and carry is None:
            from . import fused
            if state is None:
                return fused.cmix_forward(self, x)
            if not torch.is_grad_enabled() and x.dtype == torch.bfloat16:
                return fused.cmix_forward_stateful(self, x, state)
        x_last = x[:, -1]
        if carry is not None:
            xx = time_shift(x, None, carry[0]) - x
        elif state is None:
            xx = time_shift(x, layout) - x
        else:
            xx = torch.cat((state.ffn_x[self.layer_id].unsqueeze(1), x[:, :-1]), dim=1) - x
            state.ffn_x[self.layer_id].copy_(x[:, -1])
        k = x + xx * self.x_k
        k = torch.relu(self.key(k)) ** 2
        if carry is not None:
            return self.value(k), x_last
        return self.value(k)


class Block(nn.Module):
    """Pre-LN residual block (src/model.py:233-254); block 0 also owns ln0.
    args.modality_ffn = 1: the Block of VisualRWKV-v7/v7.10 (src/model.py:233-262) -- a second LayerNorm and channel mix, `ln_v` / `ffn_v`, for image
    tokens, created in the reference's order (same state-dict keys, same draws from the random stream); forward then needs `mask` (B, T, 1) bool and
    ends in x + where(mask, ffn_v(ln_v(x)), ffn(ln2(x)))."""

    def __init__(self, args, layer_id):
        super().__init__()
        self.args = args
        self.layer_id = layer_id
        modality = bool(getattr(args, "modality_ffn", 0))
        if layer_id == 0:
            self.ln0 = nn.LayerNorm(args.n_embd)
        self.ln1 = nn.LayerNorm(args.n_embd)
        self.ln2 = nn.LayerNorm(args.n_embd)
        if modality:
            self.ln_v = nn.LayerNorm(args.n_embd)
        self.att = RWKV_Tmix_x070(args, layer_id)
        self.ffn = RWKV_CMix_x070(args, layer_id)
        if modality:
            self.ffn_v = RWKV_CMix_x070(args, layer_id)

    def forward(self, x, v_first, state=None, layout=None, carry=None, mask=None):
        """carry (training across a cut): this layer's (att_x, ffn_x, S) of a TrainCarry; returns (x, v_first, the layer's next carry).
        mask (B, T, 1) bool, required with args.modality_ffn and refused without: True = image token."""
        if self.layer_id == 0:
            x = self.ln0(x)
        if (mask is None) != (getattr(self, "ffn_v", None) is None):
            raise ValueError("a Block with ffn_v (args.modality_ffn) needs the image mask; a Block without one takes none")
        if mask is not None:
            if state is not None or carry is not None:
                raise NotImplementedError("modality_ffn together with an inference state or a training carry: the carried channel-mix row "
                                          "(the LayerNorm output of the last token) would have to be re-normed per expert")
            xx, v_first = self.att(self.ln1(x), v_first, None, layout)
            x = x + xx
            x = x + torch.where(mask, self.ffn_v(self.ln_v(x), None, layout), self.ffn(self.ln2(x), None, layout))      # the reference's statement
            return x, v_first
        if carry is not None:
            if state is not None or layout is not None:
                raise NotImplementedError("a training carry together with an inference state or packed rows")
            xx, v_first, (att_x, s_end) = self.att(self.ln1(x), v_first, None, None, (carry[0], carry[2]))
            x = x + xx
            xx, ffn_x = self.ffn(self.ln2(x), None, None, (carry[1],))
            return x + xx, v_first, (att_x, ffn_x, s_end)
        if layout is not None:
            xx, v_first = self.att(self.ln1(x), v_first, None, layout)
            x = x + xx
            x = x + self.ffn(self.ln2(x), None, layout)
        elif state is None:
            xx, v_first = self.att(self.ln1(x), v_first)
            x = x + xx
            x = x + self.ffn(self.ln2(x))
        else:
            xx, v_first = self.att(self.ln1(x), v_first, state)
            x = x + xx
            x = x + self.ffn(self.ln2(x), state)
        return x, v_first


class L2Wrap(torch.autograd.Function):
    """Identity on the loss; adds 1e-4/(B*T) * max-logit at the arg-max to the logits' gradient
    (src/model.py:257-271)."""

    @staticmethod
    def forward(ctx, loss, y):
        ctx.save_for_backward(y)
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        y = ctx.saved_tensors[0]
        factor = 1e-4 / (y.shape[0] * y.shape[1])
        maxx, ids = torch.max(y, -1, keepdim=True)
        gy = torch.zeros_like(y)
        gy.scatter_(-1, ids, maxx * factor)
        return grad_output, gy


class L2WrapWindow(torch.autograd.Function):
    """L2Wrap on the logits of a window of a longer row (VisualRWKV.train_step_cut): the same gradient term with the factor of the whole
    row, 1e-4 / (B * T of the uncut row), passed in."""

    @staticmethod
    def forward(ctx, loss, y, factor):
        ctx.save_for_backward(y)
        ctx.factor = float(factor)
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        y = ctx.saved_tensors[0]
        maxx, ids = torch.max(y, -1, keepdim=True)
        gy = torch.zeros_like(y)
        gy.scatter_(-1, ids, maxx * ctx.factor)
        return grad_output, gy, None


class RWKV7State:
    """Recurrent state of an RWKV-7 stack for stateful generation (the reference re-runs the
    whole sequence per generated token, src/model.py:513-529).  Per layer: the last token fed to the time-mix and
    channel-mix shifts (the reference's ZeroPad2d shift sees zeros before the first token) and the WKV state
    S (B,H,64,64) fp32.  Whole 16-token chunks go through the chunked MFMA forward kernel continuing from S (cut into
    sequence-parallel segments when the heads alone cannot fill the chip); the ragged tail and single tokens are one
    `wkv7_step` launch each.  With `blocks` (the model's Blocks) a layer that owns a tuned initial state (`time_state`, args.state_tune)
    starts from it, broadcast over the batch, instead of from zeros."""

    def __init__(self, args, batch, device, dtype=torch.bfloat16, blocks=None):
        L, C = args.n_layer, args.n_embd
        self.att_x = [torch.zeros(batch, C, device=device, dtype=dtype) for _ in range(L)]
        self.ffn_x = [torch.zeros(batch, C, device=device, dtype=dtype) for _ in range(L)]
        self.S = [torch.zeros(batch, args.dim_att // 64, 64, 64, device=device, dtype=torch.float32) for _ in range(L)]
        self.fresh = [True] * L
        self.n_tokens = 0
        for i, blk in enumerate(blocks if blocks is not None else ()):
            ts = getattr(blk.att, "time_state", None)
            if ts is not None:
                self.S[i].copy_(ts.detach().to(device=device, dtype=torch.float32).unsqueeze(0).expand_as(self.S[i]))
                self.fresh[i] = False                   # the first chunks continue from S like every later one

    def wkv(self, layer, r, w, k, v, z, b):
        from . import wkv7
        B, T, HC = r.shape
        ops = [i.view(B, T, HC // 64, 64) for i in (w, r, k, v, z, b)]      # the op's (w,q,k,v,z,a) order
        S, outs, t0 = self.S[layer], [], 0
        if T >= CHUNK_LEN:                              # whole chunks through the chunked MFMA kernel, from the carried state
            t0 = T // CHUNK_LEN * CHUNK_LEN
            head = [i[:, :t0].contiguous() for i in ops]
            y, s_end = wkv7.wkv7_forward_tparallel(*head, None if self.fresh[layer] else S)
            S.copy_(s_end)
            outs.append(y)
        for t in range(t0, T):                          # ragged tail / single tokens: one step launch each
            outs.append(wkv7.wkv7_step(*[i[:, t].contiguous() for i in ops], S).unsqueeze(1))
        self.fresh[layer] = False
        return (outs[0] if len(outs) == 1 else torch.cat(outs, dim=1)).view(B, T, HC)


class VisualTokenCompressor(nn.Module):
    """The visual token compressor of VisualRWKV-v7/v7.03 and v7.04 (src/model.py:327-374): args.n_vtc_layer plain v7.00 Blocks (Block 0 owns ln0)
    over all image tokens of a sample, every second Block on the time-reversed sequence, then its own ln_out.  Same sub-module names, so the
    reference's state-dict keys `blocks.{i}.*`, `ln_out.*` in its order.  This is the eager statement (`.flip(1)`); the GPU path is
    fused.vtc_forward with the tail kernels.  The Blocks are built from a copy of args without state_tune / modality_ffn: the compressor has
    neither tuned states nor image experts."""

    def __init__(self, args):
        super().__init__()
        import copy
        self.args = args
        bargs = copy.copy(args)
        bargs.state_tune = 0
        bargs.modality_ffn = 0
        self.blocks = nn.ModuleList([Block(bargs, i) for i in range(args.n_vtc_layer)])
        self.ln_out = nn.LayerNorm(args.n_embd)

    def pad_left(self, x, num_tokens_to_pad):
        """ZERO rows on the left (src/model.py:334-342) -- not the EOS embedding that RWKV.pad_left uses."""
        if num_tokens_to_pad != 0:
            x = torch.cat((torch.zeros(x.size(0), num_tokens_to_pad, x.size(2), dtype=x.dtype, device=x.device), x), dim=1)
        return x

    def unpad(self, x, num_tokens_to_pad):
        return x[:, num_tokens_to_pad:] if num_tokens_to_pad > 0 else x

    def forward(self, x, layout=None, tail=None):
        """x (B, L, C) -> (B, L, C).  tail = (Lout, reduction[, embeds2d, row_index]): also compress_visual_tokens' reduction to Lout tokens ('pool' /
        'step', src/model.py:521-529); on the fused path 'pool' may write straight into rows `row_index` of the (rows, C) token embeddings
        (fused.vtc_compress), which are then returned.  Calling the module (rather than fused.vtc_forward) lets forward pre-hooks run."""
        if layout is not None:
            raise NotImplementedError("packed rows inside the compressor: a reversed Block would run every sample of the row backwards into its "
                                      "neighbour; the compressor takes one sample per row")
        if tail is not None:
            from . import fused
            Lout, reduction, *scatter = tail
            if fused.vtc_supported(self, x):
                return fused.vtc_compress(self, x, Lout, reduction, *scatter, grad_cp=getattr(self.args, "grad_cp", 0))
            if scatter:
                raise NotImplementedError("the scatter into the token embeddings is the fused path's (bf16 on the GPU, args.fused)")
            h = self.forward(x)
            if reduction == "step":
                return h[:, ::x.size(1) // Lout, :]
            if reduction != "pool":
                raise ValueError(f"reduction = {reduction!r}: 'pool' or 'step'")
            return F.adaptive_avg_pool1d(h.permute(0, 2, 1), Lout).permute(0, 2, 1)
        rem = x.size(1) % CHUNK_LEN
        num_tokens_to_pad = CHUNK_LEN - rem if rem != 0 else 0
        x = self.pad_left(x, num_tokens_to_pad)
        v_first = torch.empty_like(x)
        for i, block in enumerate(self.blocks):
            reverse = i % 2 == 1
            if reverse:             # the pad rows are ordinary rows: after a reversed Block they hold values that the next Block reads
                x, v_first = x.flip(1), v_first.flip(1)
            if getattr(self.args, "grad_cp", 0) >= 1 and torch.is_grad_enabled():
                from torch.utils.checkpoint import checkpoint
                x, v_first = checkpoint(block, x, v_first, use_reentrant=False)
            else:
                x, v_first = block(x, v_first)
            if reverse:
                x, v_first = x.flip(1), v_first.flip(1)
        return self.unpad(self.ln_out(x), num_tokens_to_pad)


class VRWKV(nn.Module):
    """The trainable RWKV vision encoder of VisualRWKV-v7/v7.10 (src/model.py:367-415): a Conv2d patch embedding, args.n_vrwkv_layer plain Blocks
    (the reference hard-codes 6 VBlocks; Block 0 owns ln0), its own ln_out, and a Linear(n_embd, 1000) ImageNet head over the mean of the tokens.
    Same sub-module names in the reference's order, so its `vrwkv.*` state-dict keys exchange strictly.  The Blocks are built from a copy of args
    without state_tune / modality_ffn but with the language model's n_layer, which the reference's VBlock also sees and the initialisation depends
    on.  This is the eager statement; the GPU path is fused.vrwkv_forward.
    The reference's pad_left calls the Conv2d with token indices, so it raises whenever the token count is no multiple of 16: VRWKV exists only
    for (image_size // patch_size)^2 % 16 == 0, which is checked here."""

    def __init__(self, args):
        super().__init__()
        import copy
        n_tok = (int(args.image_size) // int(args.patch_size)) ** 2
        if n_tok % CHUNK_LEN != 0:
            raise ValueError(f"VRWKV: (image_size // patch_size)^2 = {n_tok} tokens per image must be a multiple of {CHUNK_LEN} "
                             "(the reference cannot pad the image tokens)")
        self.args = args
        bargs = copy.copy(args)
        bargs.state_tune = 0
        bargs.modality_ffn = 0
        self.emb = nn.Conv2d(3, args.n_embd, kernel_size=args.patch_size, stride=args.patch_size)
        self.blocks = nn.ModuleList([Block(bargs, i) for i in range(int(args.n_vrwkv_layer))])
        self.ln_out = nn.LayerNorm(args.n_embd)
        self.head = nn.Linear(args.n_embd, 1000)

    def forward(self, images, scatter=None):
        """images (B_img, 3, H, W) -> (features (B_img, L, C), logits (B_img, 1000)).  scatter = (embeds2d, row_index), fused path only: the
        features are written into rows `row_index` of the (rows, C) token embeddings, which are returned in their place."""
        from . import fused
        if fused.vrwkv_supported(self, images):
            return fused.vrwkv_forward(self, images, *(scatter or ()), grad_cp=getattr(self.args, "grad_cp", 0))
        if scatter:
            raise NotImplementedError("the scatter into the token embeddings is the fused path's (bf16 on the GPU, args.fused)")
        x = self.emb(images).flatten(2).transpose(1, 2)
        if x.size(1) % CHUNK_LEN != 0:
            raise ValueError(f"VRWKV: {x.size(1)} tokens per image must be a multiple of {CHUNK_LEN}")
        v_first = torch.empty_like(x)
        for block in self.blocks:
            if getattr(self.args, "grad_cp", 0) >= 1 and torch.is_grad_enabled():
                from torch.utils.checkpoint import checkpoint
                x, v_first = checkpoint(block, x, v_first, use_reentrant=False)
            else:
                x, v_first = block(x, v_first)
        x = self.ln_out(x)
        return x, self.head(x.mean(dim=1))


class RWKV(nn.Module):
    """Embedding -> n_layer Blocks -> ln_out -> head, on already-embedded inputs (src/model.py:273-325).

    `forward(x_emb)` left-pads T to a multiple of CHUNK_LEN with emb(STOP_TOKEN_INDEX) and strips the
    pad from the logits.  `args.grad_cp` is the reference's memory-saving switch (src/model.py:318-319: deepspeed.checkpointing.checkpoint per
    Block).  1 re-computes each Block in the backward, as the reference does (eager path: torch.utils.checkpoint, fused path: the same schedule
    through the fused kernels); 2 (not in the reference; fused path) = selective recompute -- WKV7 checkpoints + relu^2 dropped, every GEMM output
    kept: a third of the activation memory saved for ~4 % of the step; on the eager path 2 falls back to 1."""

    def __init__(self, args):
        super().__init__()
        self.args = args
        self.emb = nn.Embedding(args.vocab_size, args.n_embd)
        self.blocks = nn.ModuleList([Block(args, i) for i in range(args.n_layer)])
        self.ln_out = nn.LayerNorm(args.n_embd)
        self.head = nn.Linear(args.n_embd, args.vocab_size, bias=False)
        if args.dropout > 0:
            self.drop0 = nn.Dropout(p=args.dropout)

    def pad_left(self, x, num_tokens_to_pad):
        if num_tokens_to_pad != 0:
            eos_idx = torch.full((x.size(0), num_tokens_to_pad), STOP_TOKEN_INDEX, dtype=torch.long, device=x.device)
            x = torch.cat((self.emb(eos_idx), x), dim=1)
        return x

    def unpad(self, x, num_tokens_to_pad):
        return x[:, num_tokens_to_pad:] if num_tokens_to_pad > 0 else x

    def forward_features(self, x, layout=None, carry=None, mask=None, n_image=None):
        """Everything up to (not including) the head; returns (hidden, num_tokens_to_pad).
        mask (B, T, 1) bool (args.modality_ffn; True = image token): left-padded with False like x is padded (v7.10 src/model.py:350).  n_image: the
        number of True entries when the caller counted them on the host (fused.RoutePlan then needs no device synchronisation).  layout: a wkv7.PackedLayout for packed rows
        (T is then a multiple of CHUNK_LEN by construction: no left pad).  carry: a TrainCarry when x is one segment of a longer row (T a
        multiple of CHUNK_LEN: a left pad inside a row would change it); returns (hidden, 0, the carry leaving the segment)."""
        args = self.args
        modality = bool(getattr(args, "modality_ffn", 0))
        if modality != (mask is not None):
            raise ValueError("args.modality_ffn and the image mask go together: RWKV.forward(x, mask=...) with it, no mask without")
        if mask is not None and (mask.dtype != torch.bool or tuple(mask.shape) != (x.size(0), x.size(1), 1)):
            raise ValueError(f"mask must be ({x.size(0)}, {x.size(1)}, 1) bool, got {tuple(mask.shape)} {mask.dtype}")
        if carry is not None:
            if mask is not None:
                raise NotImplementedError("a training carry together with args.modality_ffn (cut rows are not routed)")
            return self._forward_features_carry(x, layout, carry)
        if layout is not None:
            layout.check(x.size(0), x.size(1), x.device)
            if getattr(args, "state_tune", 0):
                raise NotImplementedError("packed rows together with args.state_tune: every segment would have to start from time_state")
        rem = x.size(1) % CHUNK_LEN
        num_tokens_to_pad = CHUNK_LEN - rem if rem != 0 else 0
        x = self.pad_left(x, num_tokens_to_pad)
        if mask is not None and num_tokens_to_pad:
            mask = torch.cat((torch.zeros_like(mask[:, :num_tokens_to_pad]), mask), dim=1)
        if args.dropout > 0:
            x = self.drop0(x)
        def rk():       # blocks_forward's `route` keyword, only where there is a mask: the plan is built once per batch, where a fused path takes it
            from . import fused
            return {"route": fused.RoutePlan(mask, n_image)} if mask is not None else {}
        if layout is not None and getattr(args, "fused", False):
            from . import fused
            if fused.packed_supported(x):
                return fused.blocks_forward(self, x, grad_cp=int(args.grad_cp) if torch.is_grad_enabled() else 0, layout=layout, **rk()), num_tokens_to_pad
        if layout is not None:
            # the unfused Blocks (masked shift in PyTorch, the WKV7 op packed on device tensors): CPU tensors, args.fused off, or the
            # two-kernel shift's shapes (C > 4096), whose kernels know no sample boundaries inside a row
            v_first = torch.empty_like(x)
            for block in self.blocks:
                if args.grad_cp >= 1 and torch.is_grad_enabled():
                    from torch.utils.checkpoint import checkpoint
                    x, v_first = checkpoint(block, x, v_first, None, layout, None, mask, use_reentrant=False)
                else:
                    x, v_first = block(x, v_first, None, layout, None, mask)
            return self.ln_out(x), num_tokens_to_pad
        if getattr(args, "fused", False):
            from . import fused
            if fused.add_ln_supported(x):
                return fused.blocks_forward(self, x, grad_cp=int(args.grad_cp) if torch.is_grad_enabled() else 0, **rk()), num_tokens_to_pad
        v_first = torch.empty_like(x)
        for block in self.blocks:
            if args.grad_cp >= 1 and torch.is_grad_enabled():
                from torch.utils.checkpoint import checkpoint
                x, v_first = checkpoint(block, x, v_first, None, None, None, mask, use_reentrant=False)
            else:
                x, v_first = block(x, v_first, None, None, None, mask)
        return self.ln_out(x), num_tokens_to_pad

    def _forward_features_carry(self, x, layout, carry):
        args = self.args
        if layout is not None:
            raise NotImplementedError("a training carry together with packed rows: the segments of a packed row would each need their own")
        if x.size(1) % CHUNK_LEN != 0:
            raise ValueError(f"a segment of a cut row must be a multiple of {CHUNK_LEN} tokens (got {x.size(1)})")
        if len(carry.layers) != len(self.blocks):
            raise ValueError(f"the carry has {len(carry.layers)} layers, the model {len(self.blocks)}")
        if args.dropout > 0:
            x = self.drop0(x)
        grad_cp = int(args.grad_cp) if torch.is_grad_enabled() else 0
        if getattr(args, "fused", False):
            from . import fused
            if fused.carry_supported(x):
                h, nxt = fused.blocks_forward(self, x, grad_cp=grad_cp, carry=carry)
                return h, 0, nxt
        # the unfused Blocks (the shift in PyTorch, the WKV7 state op): CPU tensors, args.fused off, the two-kernel shift, C > 4096
        v_first = torch.empty_like(x)
        layers = []
        for i, block in enumerate(self.blocks):
            if grad_cp >= 1:
                from torch.utils.checkpoint import checkpoint
                x, v_first, lc = checkpoint(block, x, v_first, None, None, carry[i], use_reentrant=False)
            else:
                x, v_first, lc = block(x, v_first, None, None, carry[i])
            layers.append(lc)
        return self.ln_out(x), 0, TrainCarry(len(layers), layers)

    def forward(self, x, hidden_only=False, layout=None, carry=None, mask=None, n_image=None):
        """Logits (B, T, V); hidden_only: forward_features(x) instead (through the module call, so that forward pre-hooks run).
        mask (B, T, 1) bool, n_image: see forward_features (args.modality_ffn).
        layout: a wkv7.PackedLayout when the rows hold several samples end to end.
        carry: a TrainCarry when x is one segment of a longer row; returns (logits, next carry), or forward_features' triple."""
        if carry is not None:
            if hidden_only:
                return self.forward_features(x, layout, carry, mask)
            x, _, nxt = self.forward_features(x, layout, carry, mask)
            if x.is_cuda and getattr(self.args, "fused", False):
                from . import fused
                return fused.linear(self.head, x), nxt
            return self.head(x), nxt
        if hidden_only:
            return self.forward_features(x, layout, None, mask, n_image)
        x, num_tokens_to_pad = self.forward_features(x, layout, None, mask, n_image)
        if x.is_cuda and getattr(self.args, "fused", False):
            from . import fused
            x = fused.linear(self.head, x)              # input gradient in the forward GEMMs' layout
        else:
            x = self.head(x)
        return self.unpad(x, num_tokens_to_pad)

    @torch.no_grad()
    def forward_stateful(self, x, state=None, last_only=False):
        """Inference on embedded tokens x (B,T,C) continuing from `state` (None: empty context).  No padding is
        added: logits equal those `forward` gives for the same absolute positions of the concatenated sequence.
        Returns (logits (B,T,V) or (B,V) with last_only, state)."""
        if getattr(self.args, "modality_ffn", 0):
            raise NotImplementedError("forward_stateful with args.modality_ffn: the carried channel-mix row is a LayerNorm output, and the next token "
                                      "would need it under ITS expert's LayerNorm (ln2 or ln_v); the state would have to carry the un-normed row")
        if state is None:
            state = RWKV7State(self.args, x.size(0), x.device, x.dtype, blocks=self.blocks)
        v_first = torch.empty_like(x)
        use_decode = False
        if getattr(self.args, "fused", False) and x.shape[1] == 1:
            from . import decode
            use_decode = decode.supported(x)
        for block in self.blocks:
            if use_decode:                               # single token: batched-GEMV step (decode.py)
                x, v_first = decode.block_decode(block, x, v_first, state)
                state.fresh[block.layer_id] = False
            else:
                x, v_first = block(x, v_first, state)
        state.n_tokens += x.size(1)
        if use_decode and self.head.weight.dtype == torch.bfloat16:
            logits = decode.head_decode(self, x)
            return (logits if last_only else logits.unsqueeze(1)), state
        if last_only:
            x = x[:, -1]
        return self.head(self.ln_out(x)), state

    def make_decoder(self, state):
        """A single-token decode step captured in a HIP graph (the eager step is ~1000 small launches for 24 layers and
        is bound by launch overhead, not by the GPU).  Returns `step(x_emb (B,1,C)) -> logits (B,V)`; `state` is
        advanced in place by every call, exactly as `forward_stateful(x_emb, state, last_only=True)` would."""
        return GraphDecoder(self, state)

    def decoder_for(self, state, sampled=False, penalised=False):
        """`make_decoder` with the captured graph re-used across prompts: one capture per (batch size, device, parameter
        versions, sampled, penalised); later calls copy `state` into the graph's own state tensors.  The returned decoder advances ITS
        state (`decoder.state`), not the argument.  sampled: the step ends in the pick kernel (GraphDecoder.sample); penalised: in the
        pick under presence / count penalties and a token ban, on the decoder's own occurrence counts (decoder.pick.occ)."""
        S0 = state.S[0]
        from . import param_state
        key = (S0.shape[0], S0.device, sum(p._version for p in self.parameters()), param_state.generation(), bool(sampled), bool(penalised))
        cache = self.__dict__.setdefault("_decoders", {})
        dec = cache.get(key)
        if dec is None:
            for k in [k for k in cache if k[:4] != key[:4]]:      # parameters changed (or first use): stale graphs go
                del cache[k]
            dec = cache[key] = GraphDecoder(self, state, sampled=sampled, penalised=penalised)
        elif dec.state is not state:
            dec.load_state(state)
        return dec


class GraphDecoder:
    """sampled=False: `__call__(x_emb) -> logits`.  sampled=True: the captured chain ends in the pick kernel (sampling.py), which turns the
    logits into the token, its logit and probability (self.pick) and writes the token's embedding row into x_in -- the next replay's input,
    in stream order; a generated token is `sample(u)`: one small device-to-device copy, one replay, one read-back.  penalised=True (with
    sampled): that last kernel is the penalised pick on self.pick.occ (B, V), the run's occurrence counts, which it updates itself;
    `self.pick.reset(token_ban)` starts a run."""
    def __init__(self, rwkv: "RWKV", state: RWKV7State, sampled=False, penalised=False):
        if penalised and not sampled:
            raise ValueError("GraphDecoder(penalised=True) goes with sampled=True: the penalties are part of the pick")
        self.rwkv, self.state, self.sampled, self.penalised = rwkv, state, sampled, penalised
        p = next(rwkv.parameters())
        B = state.S[0].shape[0]
        self.x_in = torch.zeros(B, 1, rwkv.args.n_embd, device=p.device, dtype=p.dtype)
        if sampled:
            from . import sampling
            # params, u, token, logit_prob (and the counts) at fixed addresses
            self.pick = sampling.PickBuffers(B, p.device, V=rwkv.emb.weight.size(0) if penalised else None)

            def step():
                logits, _ = rwkv.forward_stateful(self.x_in, state, last_only=True)
                if not sampling.kernel_supported(logits, rwkv.emb.weight, self.x_in):
                    raise RuntimeError("GraphDecoder(sampled=True): the pick kernel takes bf16 logits of a vocabulary that is a multiple of 8 "
                                       f"and at most {sampling.MAX_V}, and a bf16 embedding (got {tuple(logits.shape)} {logits.dtype})")
                sampling.launch_pick(logits, self.pick, rwkv.emb.weight, self.x_in, self.pick.occ)
                return logits
        else:
            def step():
                return rwkv.forward_stateful(self.x_in, state, last_only=True)[0]
        keep = [t.clone() for t in state.att_x + state.ffn_x + state.S]       # warm-up and capture run the step for real
        fresh, n_tok = list(state.fresh), state.n_tokens
        side = torch.cuda.Stream(device=p.device)
        side.wait_stream(torch.cuda.current_stream(p.device))
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(2):
                step()
        torch.cuda.current_stream(p.device).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph):
            self.logits = step()
        for dst, src in zip(state.att_x + state.ffn_x + state.S, keep):
            dst.copy_(src)
        state.fresh, state.n_tokens = fresh, n_tok
        if penalised:
            self.pick.reset()                                # warm-up and capture counted their tokens

    @torch.no_grad()
    def load_state(self, other: RWKV7State):
        """Continue from another prompt's state: copied into the tensors the graph was captured on."""
        mine = self.state
        for dst, src in zip(mine.att_x + mine.ffn_x + mine.S, other.att_x + other.ffn_x + other.S):
            dst.copy_(src)
        mine.fresh, mine.n_tokens = list(other.fresh), other.n_tokens

    @torch.no_grad()
    def __call__(self, x_emb):
        self.x_in.copy_(x_emb)
        self.graph.replay()
        self.state.n_tokens += 1
        self.state.fresh = [False] * len(self.state.fresh)
        return self.logits

    @torch.no_grad()
    def sample(self, u):
        """One generated token of the sampled decoder: u (B,) on the device -> (token int32 (B,), logit (B,), prob (B,)) on the host.  The input
        is what the previous pick (a replay's, or the caller's eager first one with x_out = x_in) left in x_in; temperature and top_p are
        what `self.pick.set` last wrote."""
        self.pick.u.copy_(u)
        self.graph.replay()
        self.state.n_tokens += 1
        self.state.fresh = [False] * len(self.state.fresh)
        return self.pick.read()
