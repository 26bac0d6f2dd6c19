"""Single-token decode step of a Block (RWKV_Tmix_x070 + RWKV_CMix_x070, src/model.py:166-194,221-227,247-254) with
carried state: 5 launches per layer instead of the ~25 the module-level stateful path issues.  Every nn.Linear and
first-stage LoRA product is a row of a batched GEMV launch with its activation / residual in the epilogue
(csrc/gemv_decode.hip); LayerNorm + token shift + lerps are folded into the GEMV that consumes them (a separate kernel
for widths the fold does not cover), and everything that is per-head -- the second
LoRA stage, decay, k/v/a glue, the WKV7 state step, GroupNorm + bonus + gate -- is another (csrc/decode_fused.hip).
Inference only; first-stage LoRA factors are read through cached (N,K)-major copies (rebuilt when a parameter is
modified in place)."""
from __future__ import annotations

import torch

from . import hip_lib

ACT_NONE, ACT_TANH, ACT_SIGMOID, ACT_RELUSQ = 0, 1, 2, 3
MAX_B = 4


def _gemv(entry, jobs, B, device, gates=None, copy=False):
    """One launch of a batched-GEMV entry of csrc/gemv_decode.hip: the one place that lays out its job arrays.  jobs: list of
    (W (N,K), x (B,K), res (B,N) or None, act); gates: the gated entry's (B,N) per job; copy: None or (src, dst) for the entries with the copy side
    job (dst[:] = src), False for the entry without.  Returns the list of y (B,N) bf16."""
    Ws, xs, res, acts = zip(*jobs)
    ys = [torch.empty(B, W.shape[0], dtype=torch.bfloat16, device=device) for W in Ws]
    args = [len(jobs), B, Ws, xs, res, ys, [W.shape[0] for W in Ws], [W.shape[1] for W in Ws], acts]
    if gates is not None:
        args.insert(5, gates)
    if copy is not False:
        args += (copy[0], copy[1], copy[0].numel()) if copy else (None, None, 0)
    hip_lib.launch(entry, *args, device=device)
    return ys


def gemv_multi(jobs, B, device, copy=None):
    """jobs: list of (W (N,K), x (B,K), res (B,N) or None, act) -> list of y (B,N) bf16, one launch.
    copy: optional (src, dst), dst[:] = src as the side job (the carried token-shift row, see gemv_ln_multi)."""
    if copy is None:
        return _gemv("vrwkv_gemv_multi_bf16", jobs, B, device)
    return _gemv("vrwkv_gemv_multi_copy_bf16", jobs, B, device, copy=copy)


def gemv_gated(jobs, B, device, copy=None):
    """jobs: list of (W (N,K), x (B,K), res (B,N) or None, gate (B,N), act) -> list of y = res + gate * act(W x), one launch.
    copy: optional (src, dst), dst[:] = src as the side job."""
    return _gemv("vrwkv_gemv_gated_copy_bf16", [(W, x, r, a) for W, x, r, _, a in jobs], B, device, gates=[j[3] for j in jobs], copy=copy)


def ln_fold_supported(C):
    return 512 <= C <= 4096 and C % 8 == 0


def gemv_ln_multi(jobs, x, ln, x_prev):
    """jobs: list of (W (N,K), mu (K), act); x (B,K) raw residual row.  y_j = act_j(W_j (h + (x_prev - h) mu_j)) with
    h = LayerNorm(x), one launch.  Returns (ys, h); x_prev is NOT updated (the caller hands h to a later launch's
    copy side job, because workgroups of this launch read x_prev until it ends)."""
    B, K = x.shape
    Ws, mus, acts = zip(*jobs)
    ys = [torch.empty(B, W.shape[0], dtype=torch.bfloat16, device=x.device) for W in Ws]
    h = torch.empty_like(x)
    hip_lib.launch("vrwkv_gemv_ln_multi_bf16", len(jobs), B, K, Ws, x, ln.weight, ln.bias, float(ln.eps), x_prev, mus, h, ys,
                   [W.shape[0] for W in Ws], acts, device=x.device)
    return ys, h


def ln_mix(x, ln, x_prev, mus):
    """x (B,C) -> [LN(x) + (x_prev - LN(x)) * mu for mu in mus]; x_prev (B,C) is replaced by LN(x) in place."""
    B, C = x.shape
    outs = [torch.empty_like(x) for _ in mus]
    hip_lib.launch("vrwkv_decode_ln_mix_bf16", B, C, len(mus), x, ln.weight, ln.bias, float(ln.eps), x_prev, list(mus), outs, device=x.device)
    return outs


def tmix_head(m, r, k, v, v_first, hidden, S, carry=None):
    """Everything of RWKV_Tmix_x070.forward between the first-stage products and the output projection, for one token.
    hidden: [tanh(xw w1), xa a1, sigmoid(xg g1)] (+ [xv v1] on layers > 0), each (B,D); S (B,H,64,64) fp32, in place.
    carry: optional (src, dst) pair of (B,C) rows copied as a side job."""
    B, C = r.shape
    names = ("w2", "a2", "g2") + (("v2",) if v_first is not None else ())
    t = _transposed(m, names, "_decode_cache2")
    W2 = [t[n] for n in names]                       # (C, D): a channel's D weights are contiguous
    out = torch.empty_like(r)
    src, dst = carry if carry else (None, None)
    hip_lib.launch("vrwkv_decode_tmix_head_bf16", B, C // 64, r, k, v, v_first, list(hidden), W2, [w.shape[1] for w in W2], m.w0, m.a0,
                   m.v0 if v_first is not None else None, m.k_k, m.k_a, m.r_k, m.ln_x.weight, m.ln_x.bias, float(m.ln_x.eps), S, out, src, dst,
                   device=r.device)
    return out


def _transposed(m, names, slot="_decode_cache"):
    """(N,K)-major copies of the LoRA factors used as `x @ p`; cached on the module, keyed by the parameters' versions."""
    from . import param_state
    key = (param_state.generation(),) + tuple((getattr(m, n).data_ptr(), getattr(m, n)._version) for n in names)
    cache = getattr(m, slot, None)
    if cache is None or cache[0] != key:
        cache = (key, {n: getattr(m, n).detach().t().contiguous() for n in names})
        setattr(m, slot, cache)
    return cache[1]


def supported(x):
    return x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 3 and x.shape[1] == 1 and x.shape[0] <= MAX_B


def _bf16_contig(m, names):
    return all(getattr(m, n).dtype == torch.bfloat16 and getattr(m, n).is_contiguous() for n in names)


@torch.no_grad()
def block_decode(block, x, v_first, state):
    """One Block (src/model.py:247-254) for one token: x (B,1,C) residual stream in, residual stream out."""
    B, _, C = x.shape
    dev = x.device
    att, ffn, lid = block.att, block.ffn, block.layer_id
    assert _bf16_contig(att, ("w0", "a0", "k_k", "k_a", "r_k")), "decode step: bf16 contiguous parameters"
    if lid == 0:
        x = block.ln0(x)
    x = x.reshape(B, C)
    t = _transposed(att, ("w1", "a1", "g1") + (("v1",) if lid > 0 else ()))
    fold = ln_fold_supported(C)                  # LayerNorm + shift + lerps inside the consuming GEMV launch
    mats = [(att.receptance.weight, att.x_r, ACT_NONE), (att.key.weight, att.x_k, ACT_NONE), (att.value.weight, att.x_v, ACT_NONE),
            (t["w1"], att.x_w, ACT_TANH), (t["a1"], att.x_a, ACT_NONE), (t["g1"], att.x_g, ACT_SIGMOID)]
    if lid > 0:
        mats.append((t["v1"], att.x_v, ACT_NONE))
    carry = None
    if fold:
        outs, h = gemv_ln_multi(mats, x, block.ln1, state.att_x[lid])
        carry = (h, state.att_x[lid])
    else:
        ins = dict(zip(("x_r", "x_w", "x_k", "x_v", "x_a", "x_g"),
                       ln_mix(x, block.ln1, state.att_x[lid], [att.x_r, att.x_w, att.x_k, att.x_v, att.x_a, att.x_g])))
        names = ["x_r", "x_k", "x_v", "x_w", "x_a", "x_g", "x_v"]
        outs = gemv_multi([(W, ins[nm], None, act) for (W, _, act), nm in zip(mats, names)], B, dev)
    r, k, v = outs[:3]
    if lid == 0:
        v_first = v.view(B, 1, C)
    y = tmix_head(att, r, k, v, v_first.view(B, C) if lid > 0 else None, outs[3:], state.S[lid], carry)
    (x,) = gemv_multi([(att.output.weight, y, x, ACT_NONE)], B, dev)                                # x + output(y)
    if fold:
        (kk,), h = gemv_ln_multi([(ffn.key.weight, ffn.x_k, ACT_RELUSQ)], x, block.ln2, state.ffn_x[lid])
        (x2,) = gemv_multi([(ffn.value.weight, kk, x, ACT_NONE)], B, dev, copy=(h, state.ffn_x[lid]))
    else:
        (kx,) = ln_mix(x, block.ln2, state.ffn_x[lid], [ffn.x_k])
        (kk,) = gemv_multi([(ffn.key.weight, kx, None, ACT_RELUSQ)], B, dev)
        (x2,) = gemv_multi([(ffn.value.weight, kk, x, ACT_NONE)], B, dev)                            # x + value(relu(key)^2)
    return x2.view(B, 1, C), v_first


@torch.no_grad()
def head_decode(rwkv, x):
    """ln_out + head for one token: x (B,1,C) -> logits (B,V).  The head is one GEMV over the (V,C) matrix."""
    B, _, C = x.shape
    h = rwkv.ln_out(x).view(B, C)
    (logits,) = gemv_multi([(rwkv.head.weight, h, None, ACT_NONE)], B, x.device)
    return logits
