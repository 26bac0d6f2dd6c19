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

`pick` launches the HIP kernel on CUDA bf16 rows and runs `pick_torch` -- the same five steps in fp32 torch -- on anything else."""
from __future__ import annotations

import torch

MAX_V = 65536         # vrwkv_sample_pick_bf16 keeps the row on chip


def check_args(temperature, top_p):
    if not temperature > 0:
        raise ValueError(f"sampling: temperature must be > 0 (got {temperature})")
    if not top_p >= 0:
        raise ValueError(f"sampling: top_p must be >= 0 (got {top_p})")


class PickBuffers:
    """The device-side arguments and results of the pick kernel for B rows, at fixed addresses (a captured graph reads and writes them):
    params = {temperature, top_p}, u (B), and one buffer of 3 B words behind token (B) int32 and logit_prob (B, 2) fp32, so that a step's
    results come back in one copy (read())."""
    def __init__(self, B, device):
        self.B = B
        self.params = torch.ones(2, device=device, dtype=torch.float32)
        self.u = torch.full((B,), 0.5, device=device, dtype=torch.float32)
        self.out = torch.zeros(3 * B, device=device, dtype=torch.float32)
        self.token = self.out[:B].view(torch.int32)
        self.logit_prob = self.out[B:].view(B, 2)

    def set(self, temperature, top_p):
        check_args(temperature, top_p)
        self.params.copy_(torch.tensor([float(temperature), float(top_p)], dtype=torch.float32))

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


def launch_pick(logits, bufs: PickBuffers, emb=None, x_out=None):
    """One launch of vrwkv_sample_pick_bf16 on `bufs` (no check of the tensors: kernel_supported is the caller's)."""
    from . import hip_lib
    B, V = logits.shape
    C = emb.size(1) if emb is not None else 8
    hip_lib.launch("vrwkv_sample_pick_bf16", B, V, C, logits, bufs.params, bufs.u, emb, x_out, bufs.token, bufs.logit_prob, device=logits.device)


def pick_torch(logits, temperature, top_p, u, emb=None, x_out=None):
    """The five steps of the module docstring in fp32 torch (fp64 for fp64 logits), on any device."""
    check_args(temperature, top_p)
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
    return token.int(), lt.view(B), prob


def pick(logits, temperature, top_p, u, emb=None, x_out=None):
    """(token int32 (B,), logit fp32 (B,), prob fp32 (B,)) for logits (B, V) and u (B,) in [0, 1); with emb (V, C) and x_out (B.., C) the row
    emb[token] is written to x_out.  CUDA bf16 contiguous rows go through the HIP kernel, anything else through pick_torch."""
    check_args(temperature, top_p)
    if (emb is None) != (x_out is None):
        raise ValueError("sampling.pick: emb and x_out go together")
    if not kernel_supported(logits, emb, x_out):
        return pick_torch(logits, temperature, top_p, u, emb, x_out)
    bufs = PickBuffers(logits.size(0), logits.device)
    bufs.set(temperature, top_p)
    bufs.u.copy_(torch.as_tensor(u, dtype=torch.float32).reshape(-1))
    launch_pick(logits, bufs, emb, x_out)
    return bufs.token, bufs.logit_prob[:, 0], bufs.logit_prob[:, 1]
