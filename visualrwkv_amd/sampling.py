"""Top-p / temperature sampling of one token per logits row: what the reference's applications do with the logits of
`VisualRWKV.generate`'s model pass (VisualRWKV-v7/v7.00/src/model.py:496-530 raises on do_sample; VisualRWKV-v5/v5.3/app/app_gpu.py:77
calls PIPELINE.sample_logits of the `rwkv` package).  The contract (include/visualrwkv_hip.h, vrwkv_sample_pick_bf16), for a row l,
a temperature > 0, a top_p >= 0 and a uniform number u in [0, 1):

  1. p = softmax(l) at temperature 1.
  2. K = { i : p_i >= c }, c the first value in descending order whose running sum reaches top_p.  Ties with c are kept; top_p = 0 is the
     maximum and its ties; top_p >= 1 is every token (sample_logits' argmax(cumsum >= top_p) turns into greedy when rounding keeps the
     sum below 1: not copied).
  3. q_i = p_i^(1 / temperature) on K, i.e. exp((l_i - max l) / temperature).
  4. token = the first i in K, in index order, with sum_{j <= i, j in K} q_j > u sum_K q: an inverse CDF on a caller-supplied u instead of
     torch.multinomial, so that a run can be repeated.  If rounding lets no prefix exceed the target: the last member of K of weight > 0.
  5. Beside the token: l_token, and p_token = the full-vocabulary, temperature-1 probability, both fp32.

Presence / count penalties and a token ban (vrwkv_sample_pick_pen_bf16; VisualRWKV-v7/v7.10/app/app_gpu.py:56-86 apply them around
sample_logits): with occ (B, V) fp32, the occurrence counts, a row is first turned into l': -inf where occ < 0 (banned), l - (presence + occ count)
rounded to the logits' dtype where occ > 0; the five steps run on l' (l_token and p_token are l''s); then occ decays where it is > 0 and
the token's count grows by 1.  occ is updated in place.

`pick` launches the HIP kernel on CUDA bf16 rows and runs `pick_torch` -- the same steps in fp32 torch -- on anything else."""
from __future__ import annotations

import math

import torch

MAX_V = 65536         # vrwkv_sample_pick_bf16 keeps the row on chip


def check_args(temperature, top_p, presence=0.0, count=0.0, decay=0.996, token_ban=(), V=None):
    if not temperature > 0:
        raise ValueError(f"sampling: temperature must be > 0 (got {temperature})")
    if not top_p >= 0:
        raise ValueError(f"sampling: top_p must be >= 0 (got {top_p})")
    for name, v in (("presence", presence), ("count", count)):
        if not (v >= 0 and math.isfinite(v)):
            raise ValueError(f"sampling: the {name} penalty must be finite and >= 0 (got {v})")
    if not 0 < decay <= 1:
        raise ValueError(f"sampling: the penalty decay must lie in (0, 1] (got {decay})")
    for t in token_ban:
        if int(t) != t or not (0 <= t and (V is None or t < V)):
            raise ValueError(f"sampling: banned token {t} is not an index of the vocabulary" + ("" if V is None else f" [0, {V})"))


def penalised(presence, count, token_ban):
    """Whether a call needs the occurrence counts at all: with no penalty and no ban every path is the plain pick."""
    return bool(presence or count or len(token_ban))


def reset_occ(occ, token_ban=()):
    """occ (B, V) for a new run: no token has occurred, and the banned ones (count -1) never will."""
    check_args(1.0, 1.0, token_ban=token_ban, V=occ.size(1))
    occ.zero_()
    if len(token_ban):
        occ[:, torch.as_tensor([int(t) for t in token_ban], dtype=torch.long, device=occ.device)] = -1.0
    return occ


class PickBuffers:
    """The device-side arguments and results of the pick kernel for B rows, at fixed addresses (a captured graph reads and writes them):
    params = {temperature, top_p, presence, count, decay} (the plain entry reads the first two), u (B), and one buffer of 3 B words behind
    token (B) int32 and logit_prob (B, 2) fp32, so that a step's results come back in one copy (read()).  V: the occurrence counts
    occ (B, V) fp32 of the penalised entry as well (reset())."""
    def __init__(self, B, device, V=None):
        self.B = B
        self.params = torch.tensor([1.0, 1.0, 0.0, 0.0, 1.0], device=device, dtype=torch.float32)
        self.occ = torch.zeros(B, V, device=device, dtype=torch.float32) if V is not None else None
        self.u = torch.full((B,), 0.5, device=device, dtype=torch.float32)
        self.out = torch.zeros(3 * B, device=device, dtype=torch.float32)
        self.token = self.out[:B].view(torch.int32)
        self.logit_prob = self.out[B:].view(B, 2)

    def set(self, temperature, top_p, presence=0.0, count=0.0, decay=0.996):
        check_args(temperature, top_p, presence, count, decay)
        self.params.copy_(torch.tensor([float(temperature), float(top_p), float(presence), float(count), float(decay)], dtype=torch.float32))

    def reset(self, token_ban=()):
        """A new run on the buffers' own occ (reset_occ)."""
        reset_occ(self.occ, token_ban)

    def read(self):
        """(token (B) int32, logit (B) fp32, prob (B) fp32) on the host: the step's one synchronisation."""
        host = self.out.cpu()
        B = self.B
        return host[:B].view(torch.int32), host[B::2], host[B + 1::2]


def kernel_supported(logits, emb=None, x_out=None):
    ok = (logits.is_cuda and logits.dtype == torch.bfloat16 and logits.dim() == 2 and logits.is_contiguous()
          and logits.size(1) % 8 == 0 and logits.size(1) <= MAX_V)
    if ok and emb is not None:
        ok = (emb.is_cuda and emb.dtype == torch.bfloat16 and emb.is_contiguous() and emb.size(1) % 8 == 0 and emb.size(0) == logits.size(1)
              and (x_out is None or (x_out.is_cuda and x_out.dtype == torch.bfloat16 and x_out.is_contiguous()
                                     and x_out.numel() == logits.size(0) * emb.size(1))))
    return ok


def launch_pick(logits, bufs: PickBuffers, emb=None, x_out=None, occ=None):
    """One launch of vrwkv_sample_pick_bf16 on `bufs`, or with occ (B, V) fp32 of vrwkv_sample_pick_pen_bf16 (no check of the tensors:
    kernel_supported is the caller's)."""
    from . import hip_lib
    B, V = logits.shape
    C = emb.size(1) if emb is not None else 8
    if occ is not None:
        hip_lib.launch("vrwkv_sample_pick_pen_bf16", B, V, C, logits, bufs.params, bufs.u, occ, emb, x_out, bufs.token, bufs.logit_prob,
                       device=logits.device)
        return
    hip_lib.launch("vrwkv_sample_pick_bf16", B, V, C, logits, bufs.params, bufs.u, emb, x_out, bufs.token, bufs.logit_prob, device=logits.device)


def check_occ(occ, logits):
    if occ.dtype != torch.float32 or occ.shape != logits.shape or occ.device != logits.device or not occ.is_contiguous():
        raise ValueError(f"sampling: occ must be contiguous fp32 of the logits' shape {tuple(logits.shape)} on their device "
                         f"(got {tuple(occ.shape)} {occ.dtype} on {occ.device})")


def penalise_torch(logits, occ, presence, count):
    """l' of the module docstring: the row under its counts, in the logits' dtype (the subtraction in fp32, rounded once)."""
    pen = presence + occ * count
    lp = torch.where(occ > 0, (logits.float() - pen).to(logits.dtype) if logits.dtype != torch.float64 else logits - pen.double(), logits)
    return torch.where(occ < 0, torch.full_like(lp, -math.inf), lp)


def pick_torch(logits, temperature, top_p, u, emb=None, x_out=None, occ=None, presence=0.0, count=0.0, decay=0.996):
    """The five steps of the module docstring in fp32 torch (fp64 for fp64 logits), on any device; with occ on the penalised row, and occ
    updated in place."""
    check_args(temperature, top_p, presence, count, decay)
    if occ is not None:
        check_occ(occ, logits)
        logits = penalise_torch(logits, occ, float(presence), float(count))
    l = logits if logits.dtype == torch.float64 else logits.float()
    B, V = l.shape
    u = torch.as_tensor(u, device=l.device).to(l.dtype).reshape(B, 1)
    m = l.max(dim=-1, keepdim=True).values
    e = torch.exp(l - m)
    Z = e.sum(dim=-1, keepdim=True)
    if top_p >= 1:
        K = torch.ones_like(l, dtype=torch.bool)
    else:
        ls, order = torch.sort(l, dim=-1, descending=True)
        reach = torch.cumsum(torch.gather(e, -1, order), dim=-1) >= top_p * Z
        reach[:, -1] = True                                  # rounding kept the whole sum below top_p Z: every token
        cut = torch.gather(ls, -1, reach.int().argmax(dim=-1, keepdim=True))
        K = l >= cut
    q = torch.where(K, torch.exp((l - m) / temperature), torch.zeros_like(l))
    cdf = torch.cumsum(q, dim=-1)
    ok = q > 0
    hit = ok & (cdf > u * cdf[:, -1:])
    idx = torch.arange(V, device=l.device).expand(B, V)
    first = torch.where(hit, idx, torch.full_like(idx, V)).min(dim=-1).values
    last = torch.where(ok, idx, torch.full_like(idx, -1)).max(dim=-1).values
    token = torch.where(first < V, first, last).clamp_(0, V - 1)
    lt = torch.gather(l, -1, token.view(B, 1))
    prob = (torch.exp(lt - m) / Z).view(B)
    if emb is not None:
        x_out.view(B, -1).copy_(emb[token])
    if occ is not None:
        occ.copy_(torch.where(occ > 0, occ * float(decay), occ))
        rows = torch.nonzero((q > 0).any(dim=-1)).view(-1)              # a row without weight (undefined) updates nothing
        occ[rows, token[rows]] += 1.0
    return token.int(), lt.view(B), prob


def pick(logits, temperature, top_p, u, emb=None, x_out=None, occ=None, presence=0.0, count=0.0, decay=0.996):
    """(token int32 (B,), logit fp32 (B,), prob fp32 (B,)) for logits (B, V) and u (B,) in [0, 1); with emb (V, C) and x_out (B.., C) the row
    emb[token] is written to x_out; with occ (B, V) fp32 the pick runs under the penalties and the ban of the module docstring and updates
    occ in place.  CUDA bf16 contiguous rows go through the HIP kernel, anything else through pick_torch."""
    check_args(temperature, top_p, presence, count, decay)
    if (emb is None) != (x_out is None):
        raise ValueError("sampling.pick: emb and x_out go together")
    if occ is not None:
        check_occ(occ, logits)
    if not kernel_supported(logits, emb, x_out):
        return pick_torch(logits, temperature, top_p, u, emb, x_out, occ, presence, count, decay)
    bufs = PickBuffers(logits.size(0), logits.device)
    bufs.set(temperature, top_p, presence, count, decay)
    bufs.u.copy_(torch.as_tensor(u, dtype=torch.float32).reshape(-1))
    launch_pick(logits, bufs, emb, x_out, occ)
    return bufs.token, bufs.logit_prob[:, 0], bufs.logit_prob[:, 1]
