"""Host-side mirror of the reference's RWKV-6 modules (VisualRWKV-v6/v6.0/src/model.py:92-226): same class names,
constructor arguments, parameter names and initialisers (=> the reference's state-dict keys), forward through
RUN_CUDA_RWKV6.  BASELINE config 4 (VisualRWKV-6 7B) runs the same Block/RWKV/VisualRWKV scaffolding around these."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import wkv6 as _wkv6


def _lora_mm(x, w):
    """x @ w for a LoRA factor; on the GPU under autograd the weight gradient runs in csrc/lora_wgrad.h (fused.lora_mm)."""
    if x.is_cuda and torch.is_grad_enabled():
        from .fused import lora_mm
        return lora_mm(x, w)
    return x @ w


def time_shift(x):
    """nn.ZeroPad2d((0, 0, 1, -1)): x[t-1], zero at t = 0."""
    return F.pad(x, (0, 0, 1, -1))


def _behind(prev, x):
    """The carried row `prev` (B,C) put in front of x (B,T,C): the stateful paths run the modules' own shift code over T + 1 rows and
    drop the first, whose shift read the zero pad."""
    return torch.cat((prev.unsqueeze(1).to(x.dtype), x), dim=1)


class RWKV6State:
    """Recurrent state of an RWKV-6 stack for stateful generation (the reference re-runs the whole text pass per generated token,
    v6.xx/src/model.py:468-495).  Per layer: the last ln1 / ln2 rows the time-mix and channel-mix shifts read (the reference's ZeroPad2d
    shift sees zeros before the first token) and the WKV state S (B,H,64,64) fp32 [key][value], the layout of RUN_CUDA_RWKV6_STATE."""

    def __init__(self, args, batch, device, dtype=torch.bfloat16):
        L, C = args.n_layer, args.n_embd
        self.att_x = [torch.zeros(batch, C, device=device, dtype=dtype) for _ in range(L)]
        self.ffn_x = [torch.zeros(batch, C, device=device, dtype=dtype) for _ in range(L)]
        self.S = [torch.zeros(batch, args.dim_att // args.head_size_a, args.head_size_a, args.head_size_a, device=device, dtype=torch.float32)
                  for _ in range(L)]
        self.fresh = [True] * L                 # kept for rwkv7.GraphDecoder, which saves and restores it; WKV6 starts from S whatever it holds
        self.n_tokens = 0


class RWKV_Tmix_x060(nn.Module):
    """RWKV-6 time-mix with the 5-way data-dependent token-shift LoRA (model.py:92-194)."""

    def __init__(self, args, layer_id):
        super().__init__()
        self.args = args
        self.layer_id = layer_id
        self.head_size = args.head_size_a
        self.n_head = args.dim_att // self.head_size
        assert args.dim_att % self.n_head == 0
        C, A = args.n_embd, args.dim_att
        with torch.no_grad():
            r01 = layer_id / (args.n_layer - 1)
            r10 = 1.0 - (layer_id / args.n_layer)
            ddd = (torch.arange(C, dtype=torch.float32) / C).view(1, 1, C)
            self.time_maa_x = nn.Parameter(1.0 - torch.pow(ddd, r10))
            self.time_maa_w = nn.Parameter(1.0 - torch.pow(ddd, r10))
            self.time_maa_k = nn.Parameter(1.0 - torch.pow(ddd, r10))
            self.time_maa_v = nn.Parameter(1.0 - (torch.pow(ddd, r10) + 0.3 * r01))
            self.time_maa_r = nn.Parameter(1.0 - torch.pow(ddd, 0.5 * r10))
            self.time_maa_g = nn.Parameter(1.0 - torch.pow(ddd, 0.5 * r10))
            d_mix = 64 if C >= 4096 else 32
            self.time_maa_w1 = nn.Parameter(torch.zeros(C, d_mix * 5))
            self.time_maa_w2 = nn.Parameter(torch.zeros(5, d_mix, C).uniform_(-0.01, 0.01))
            n = torch.arange(A, dtype=torch.float32)
            self.time_decay = nn.Parameter((-6 + 5 * (n / (A - 1)) ** (0.7 + 1.3 * r01)).reshape(1, 1, A))
            d_decay = 128 if C >= 4096 else 64
            self.time_decay_w1 = nn.Parameter(torch.zeros(C, d_decay))
            self.time_decay_w2 = nn.Parameter(torch.zeros(d_decay, A).uniform_(-0.01, 0.01))
            zigzag = ((torch.arange(A) + 1) % 3 - 1).float() * 0.1
            self.time_faaaa = nn.Parameter((r01 * (1 - n / (A - 1)) + zigzag).reshape(self.n_head, self.head_size))
        self.receptance = nn.Linear(C, A, bias=False)
        self.key = nn.Linear(C, A, bias=False)
        self.value = nn.Linear(C, A, bias=False)
        self.output = nn.Linear(A, C, bias=False)
        self.gate = nn.Linear(C, A, bias=False)
        self.ln_x = nn.GroupNorm(self.n_head, A, eps=(1e-5) * (args.head_size_divisor ** 2))

    def mix(self, x):
        B, T, C = x.size()
        xx = time_shift(x) - x
        xxx = x + xx * self.time_maa_x
        xxx = torch.tanh(_lora_mm(xxx, self.time_maa_w1)).view(B * T, 5, -1).transpose(0, 1)
        xxx = torch.bmm(xxx, self.time_maa_w2).view(5, B, T, -1)
        mw, mk, mv, mr, mg = xxx.unbind(dim=0)
        xw = x + xx * (self.time_maa_w + mw)
        xk = x + xx * (self.time_maa_k + mk)
        xv = x + xx * (self.time_maa_v + mv)
        xr = x + xx * (self.time_maa_r + mr)
        xg = x + xx * (self.time_maa_g + mg)
        r = self.receptance(xr)
        k = self.key(xk)
        v = self.value(xv)
        g = F.silu(self.gate(xg))
        w = self.time_decay + _lora_mm(torch.tanh(_lora_mm(xw, self.time_decay_w1)), self.time_decay_w2)
        return r, k, v, g, w

    def forward(self, x, wkv=None):
        B, T, C = x.size()
        if getattr(self.args, "fused", False):
            from . import fused
            if fused.supported6(x, self) and self.receptance.weight.dtype == torch.bfloat16:
                return fused.tmix6_forward(self, x, wkv)
        r, k, v, g, w = self.mix(x)
        run = wkv if wkv is not None else _wkv6.RUN_CUDA_RWKV6
        y = run(B, T, C, self.n_head, r, k, v, w, self.time_faaaa)
        y = self.ln_x(y.view(B * T, C)).view(B, T, C)
        return self.output(y * g)

    def forward_state(self, x, state, wkv=None, want_state=True):
        """RWKV_Tmix_x060_state.forward of VisualRWKV-v6/v6.xx/src/model.py:137-144 (same parameters as `forward`): the WKV starts
        from `state` ((B,H,64,64) f32 [key][value]; None = zeros) and the state it ends in is returned.  `wkv`: a callable with
        RUN_CUDA_RWKV6_STATE's signature.  want_state=False (product op only) leaves the final state unwritten and returns None."""
        B, T, C = x.size()
        if getattr(self.args, "fused", False):
            from . import fused
            if fused.supported6(x, self) and self.receptance.weight.dtype == torch.bfloat16:
                return fused.tmix6_forward(self, x, wkv, state=state, want_state=want_state)
        r, k, v, g, w = self.mix(x)
        if wkv is not None:
            y, state = wkv(B, T, C, self.n_head, r, k, v, w, self.time_faaaa, state)
        else:
            y, state = _wkv6.RUN_CUDA_RWKV6_STATE(B, T, C, self.n_head, r, k, v, w, self.time_faaaa, state, want_state)
        y = self.ln_x(y.view(B * T, C)).view(B, T, C)
        return self.output(y * g), state

    @torch.no_grad()
    def forward_stateful(self, x, state, wkv=None):
        """forward_state continuing from `state` (an RWKV6State), any T: the shift's first row is the carried one, the WKV starts from the
        carried S; both are replaced in place.  Plain module glue around RUN_CUDA_RWKV6_STATE (or `wkv`, same signature)."""
        B, T, C = x.size()
        lid = self.layer_id
        r, k, v, g, w = [t[:, 1:].contiguous() for t in self.mix(_behind(state.att_x[lid], x))]
        state.att_x[lid].copy_(x[:, -1])
        run = wkv if wkv is not None else _wkv6.RUN_CUDA_RWKV6_STATE
        y, S = run(B, T, C, self.n_head, r, k, v, w, self.time_faaaa, state.S[lid])
        state.S[lid].copy_(S)
        y = self.ln_x(y.view(B * T, C)).view(B, T, C)
        return self.output(y * g)


class RWKV_CMix_x060(nn.Module):
    """RWKV-6 channel-mix with the receptance gate (model.py:198-226)."""

    def __init__(self, args, layer_id):
        super().__init__()
        self.args = args
        self.layer_id = layer_id
        C = args.n_embd
        with torch.no_grad():
            r10 = 1.0 - (layer_id / args.n_layer)
            ddd = (torch.arange(C, dtype=torch.float32) / C).view(1, 1, C)
            self.time_maa_k = nn.Parameter(1.0 - torch.pow(ddd, r10))
            self.time_maa_r = nn.Parameter(1.0 - torch.pow(ddd, r10))
        self.key = nn.Linear(C, args.dim_ffn, bias=False)
        self.receptance = nn.Linear(C, C, bias=False)
        self.value = nn.Linear(args.dim_ffn, C, bias=False)

    def forward(self, x):
        if getattr(self.args, "fused", False):
            from . import fused
            if fused.supported6(x) and self.key.weight.dtype == torch.bfloat16:
                return fused.cmix6_forward(self, x)
        xx = time_shift(x) - x
        xk = x + xx * self.time_maa_k
        xr = x + xx * self.time_maa_r
        k = torch.relu(self.key(xk)) ** 2
        return torch.sigmoid(self.receptance(xr)) * self.value(k)

    @torch.no_grad()
    def forward_stateful(self, x, state):
        """forward with the shift's first row read from `state` (an RWKV6State), which then carries x's last row."""
        lid = self.layer_id
        y = self.forward(_behind(state.ffn_x[lid], x))[:, 1:]
        state.ffn_x[lid].copy_(x[:, -1])
        return y


class Block(nn.Module):
    """Pre-LN residual block of RWKV-6 (model.py:233-258); block 0 also owns ln0."""

    def __init__(self, args, layer_id):
        super().__init__()
        self.args = args
        self.layer_id = layer_id
        self.ln1 = nn.LayerNorm(args.n_embd)
        self.ln2 = nn.LayerNorm(args.n_embd)
        if layer_id == 0:
            self.ln0 = nn.LayerNorm(args.n_embd)
        self.att = RWKV_Tmix_x060(args, layer_id)
        self.ffn = RWKV_CMix_x060(args, layer_id)
        if args.dropout > 0:
            self.drop0 = nn.Dropout(p=args.dropout)
            self.drop1 = nn.Dropout(p=args.dropout)

    def forward(self, x, wkv=None):
        if self.layer_id == 0:
            x = self.ln0(x)
        if getattr(self.args, "fused", False) and self.args.dropout == 0:
            from . import fused
            if fused.supported6(x) and fused.add_ln_supported(x) and self.ln1.weight.dtype == torch.bfloat16:
                _, h = fused.add_ln(x, None, self.ln1)                         # LayerNorm kernel; the attention's residual add is
                x, h = fused.add_ln(x, self.att(h, wkv), self.ln2)            # fused with ln2 (csrc/ln_fused.hip)
                return x + self.ffn(h)
        x = x + self.att(self.ln1(x), wkv)
        x = x + self.ffn(self.ln2(x))
        return x

    def forward_state(self, x, state, wkv=None, want_state=True):
        """Block.forward of v6.xx (model.py:202-210): -> (x, state)."""
        if self.layer_id == 0:
            x = self.ln0(x)
        xx, state = self.att.forward_state(self.ln1(x), state, wkv, want_state)
        x = x + xx
        x = x + self.ffn(self.ln2(x))
        return x, state

    @torch.no_grad()
    def forward_stateful(self, x, state, wkv=None):
        """Block.forward on x (B,T,C) continuing from `state` (an RWKV6State, advanced in place): the module path of stateful inference."""
        if self.layer_id == 0:
            x = self.ln0(x)
        x = x + self.att.forward_stateful(self.ln1(x), state, wkv)
        return x + self.ffn.forward_stateful(self.ln2(x), state)


class RWKV(nn.Module):
    """Embedding -> n_layer Blocks -> ln_out -> head (model.py:277-325); same state-dict keys as the reference."""

    def __init__(self, args):
        super().__init__()
        self.args = args
        self.emb = nn.Embedding(args.vocab_size, args.n_embd)
        self.blocks = nn.ModuleList([Block(args, i) for i in range(args.n_layer)])
        self.ln_out = nn.LayerNorm(args.n_embd)
        self.head = nn.Linear(args.n_embd, args.vocab_size, bias=False)
        if args.dropout > 0:
            self.drop0 = nn.Dropout(p=args.dropout)

    def forward(self, x, wkv=None):
        args = self.args
        if args.dropout > 0:
            x = self.drop0(x)
        if getattr(args, "fused", False) and args.dropout == 0:
            from . import fused
            if fused.supported6(x) and fused.add_ln_supported(x) and self.head.weight.dtype == torch.bfloat16:
                h = fused.blocks6_forward(self, x, wkv, grad_cp=args.grad_cp >= 1 and torch.is_grad_enabled())
                return fused.linear(self.head, h)
        for block in self.blocks:
            if args.grad_cp >= 1 and torch.is_grad_enabled():      # 2 (the v7 fused path's selective mode) means 1 here
                from torch.utils.checkpoint import checkpoint
                x = checkpoint(block, x, wkv, use_reentrant=False)
            else:
                x = block(x, wkv)
        return self.head(self.ln_out(x))

    def forward_state(self, x, x_emb, wkv=None):
        """The Block loop of v6.xx's unidirectional_forward (model.py:326-343) + ln_out (no head): every Block first runs over the projected
        image features `x_emb` from a zero state, then over the text `x` from the state that pass ended in.  The image takes no context
        tokens, and its projector is reached only through dL/dS.  The text pass's own final state is not requested."""
        args = self.args
        if getattr(args, "fused", False) and args.dropout == 0:
            from . import fused
            if fused.supported6(x) and fused.add_ln_supported(x) and self.head.weight.dtype == torch.bfloat16:
                return fused.blocks6_forward_state(self, x, x_emb, wkv, grad_cp=args.grad_cp >= 1 and torch.is_grad_enabled())
        for block in self.blocks:
            if args.grad_cp >= 1 and torch.is_grad_enabled():      # the two passes of a Block are checkpointed separately (model.py:334-336)
                from torch.utils.checkpoint import checkpoint
                x_emb, state = checkpoint(block.forward_state, x_emb, None, wkv, use_reentrant=False)
                x, _ = checkpoint(block.forward_state, x, state, wkv, False, use_reentrant=False)
            else:
                x_emb, state = block.forward_state(x_emb, None, wkv)
                x, _ = block.forward_state(x, state, wkv, False)
        return self.ln_out(x)

    @torch.no_grad()
    def forward_stateful(self, x, state=None, last_only=False, wkv=None):
        """Inference on embedded tokens x (B,T,C) continuing from `state` (None: empty context, zero WKV states).  Logits equal those
        `forward` gives for the same positions of the concatenated sequence; WKV6 takes any T, so nothing is padded.  One token on the GPU
        with args.fused goes through the batched-GEMV step (decode6.py); everything else through the module path around
        RUN_CUDA_RWKV6_STATE (`wkv`: a callable with its signature; tests pass the oracle).  Returns (logits (B,T,V), or (B,V) with
        last_only; state)."""
        if state is None:
            state = RWKV6State(self.args, x.size(0), x.device, x.dtype)
        use_decode = False
        if getattr(self.args, "fused", False) and x.shape[1] == 1 and wkv is None:
            from . import decode6
            use_decode = decode6.supported(x) and self.head.weight.dtype == torch.bfloat16
        for block in self.blocks:
            x = decode6.block_decode(block, x, state) if use_decode else block.forward_stateful(x, state, wkv)
        state.n_tokens += x.size(1)
        state.fresh = [False] * len(state.fresh)
        if use_decode:
            logits = decode6.head_decode(self, x)
            return (logits if last_only else logits.unsqueeze(1)), state
        if last_only:
            x = x[:, -1]
        return self.head(self.ln_out(x)), state

    def make_decoder(self, state):
        """A single-token decode step captured in a HIP graph on one stream (the step is a chain: the graph has no parallel branches).
        Returns `step(x_emb (B,1,C)) -> logits (B,V)`; `state` is advanced in place by every call, exactly as
        `forward_stateful(x_emb, state, last_only=True)` would."""
        from .rwkv7 import GraphDecoder
        return GraphDecoder(self, state)

    def decoder_for(self, state):
        """`make_decoder` with the captured graph re-used across prompts: one capture per (batch size, device, parameter versions);
        later calls copy `state` into the graph's own state tensors (GraphDecoder.load_state).  The returned decoder advances ITS state
        (`decoder.state`), not the argument."""
        from . import param_state
        from .rwkv7 import GraphDecoder
        S0 = state.S[0]
        key = (S0.shape[0], S0.device, sum(p._version for p in self.parameters()), param_state.generation())
        cache = self.__dict__.setdefault("_decoders", {})
        dec = cache.get(key)
        if dec is None:
            cache.clear()                                 # parameters changed (or first use): stale graphs go
            dec = cache[key] = GraphDecoder(self, state)
        elif dec.state is not state:
            dec.load_state(state)
        return dec
