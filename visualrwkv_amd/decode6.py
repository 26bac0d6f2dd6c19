"""Single-token decode step of an RWKV-6 Block (RWKV_Tmix_x060 + RWKV_CMix_x060, VisualRWKV-v6/v6.0/src/model.py:92-226, with the carried
WKV state of v6.xx/src/model.py:137-144): seven launches per layer at 512 <= C <= 4096.

    1  gemv_ln_multi   ln1 + the static lerp time_maa_x + tanh(. time_maa_w1)               -> hid (B,5 D), h = ln1(x)
    2  ddlerp          the five data-dependent lerps from h, the carried row, hid and time_maa_w2; the carried row becomes h
    3  gemv_multi      receptance, key, value, gate (raw) and tanh(. time_decay_w1), five jobs
    4  tmix6_head      decay LoRA second stage, the WKV6 state step, ln_x, * silu(gate)     (per head)
    5  gemv_multi      x + output(.)
    6  gemv_ln_multi   ln2 + its two static lerps: relu(key)^2 and sigmoid(receptance)      -> h2 = ln2(x)
    7  gemv_gated      x + sigmoid(..) * value(..), the carried channel-mix row becomes h2 as the side job

Widths the LayerNorm fold does not cover (C < 512, C > 4096) spend a separate ln_mix launch for 1 and 6.  Inference only; the first LoRA
factors are read through cached (N,K)-major copies (decode._transposed), time_maa_w2 and time_decay_w2 as stored."""
from __future__ import annotations

import torch

from . import decode, hip_lib
from .decode import (ACT_NONE, ACT_RELUSQ, ACT_SIGMOID, ACT_TANH, _bf16_contig, _transposed, gemv_gated, gemv_ln_multi, gemv_multi, head_decode,  # noqa: F401
                     ln_fold_supported, ln_mix)

MAX_C = 8192
MAA = ("time_maa_w", "time_maa_k", "time_maa_v", "time_maa_r", "time_maa_g")       # the order of time_maa_w2's first dimension


def supported(x):
    """x (B,1,C): one bf16 token per sample on the GPU, within the kernels' bounds (those of fused.supported6's width)."""
    return decode.supported(x) and x.shape[2] % 64 == 0 and x.shape[2] <= MAX_C


def ddlerp(att, h, x_prev, hid):
    """The five inputs xw, xk, xv, xr, xg of RWKV_Tmix_x060.mix for one token; x_prev (B,C) is replaced by h in place."""
    B, C = h.shape
    outs = [torch.empty_like(h) for _ in MAA]
    hip_lib.launch("vrwkv_decode6_ddlerp_bf16", B, C, att.time_maa_w2.shape[1], h, x_prev, hid, att.time_maa_w2, [getattr(att, n) for n in MAA], outs,
                   device=h.device)
    return outs


def tmix_head(att, r, k, v, g, hid, S):
    """Everything of RWKV_Tmix_x060.forward between the projections and the output projection, for one token; S in place."""
    B, C = r.shape
    out = torch.empty_like(r)
    hip_lib.launch("vrwkv_decode6_tmix_head_bf16", B, C // 64, att.time_decay_w2.shape[0], r, k, v, g, hid, att.time_decay_w2, att.time_decay,
                   att.time_faaaa, att.ln_x.weight, att.ln_x.bias, float(att.ln_x.eps), S, out, device=r.device)
    return out


@torch.no_grad()
def block_decode(block, x, state):
    """One Block (v6.0/src/model.py:233-258) for one token: x (B,1,C) residual stream in, residual stream out; `state` (an RWKV6State)
    is advanced in place."""
    B, _, C = x.shape
    dev = x.device
    att, ffn, lid = block.att, block.ffn, block.layer_id
    assert att.key.weight.shape[0] == C, "decode step: dim_att == n_embd"
    assert _bf16_contig(att, MAA + ("time_maa_x", "time_maa_w2", "time_decay", "time_decay_w2", "time_faaaa")) and \
        _bf16_contig(ffn, ("time_maa_k", "time_maa_r")), "decode step: bf16 contiguous parameters"
    if lid == 0:
        x = block.ln0(x)
    x = x.reshape(B, C)
    t = _transposed(att, ("time_maa_w1", "time_decay_w1"))
    fold = ln_fold_supported(C)                  # LayerNorm + shift + lerps inside the consuming GEMV launch
    if fold:
        (hid,), h = gemv_ln_multi([(t["time_maa_w1"], att.time_maa_x, ACT_TANH)], x, block.ln1, state.att_x[lid])
    else:
        h = state.att_x[lid].clone()             # ln_mix replaces its carried row; the carried row itself is still ddlerp's input
        (xxx,) = ln_mix(x, block.ln1, h, [att.time_maa_x])
        (hid,) = gemv_multi([(t["time_maa_w1"], xxx, None, ACT_TANH)], B, dev)
    xw, xk, xv, xr, xg = ddlerp(att, h, state.att_x[lid], hid)
    r, k, v, g, dh = gemv_multi([(att.receptance.weight, xr, None, ACT_NONE), (att.key.weight, xk, None, ACT_NONE),
                                 (att.value.weight, xv, None, ACT_NONE), (att.gate.weight, xg, None, ACT_NONE),
                                 (t["time_decay_w1"], xw, None, ACT_TANH)], B, dev)
    y = tmix_head(att, r, k, v, g, dh, state.S[lid])
    (x,) = gemv_multi([(att.output.weight, y, x, ACT_NONE)], B, dev)                                # x + output(y)
    if fold:
        (kk, rr), h2 = gemv_ln_multi([(ffn.key.weight, ffn.time_maa_k, ACT_RELUSQ), (ffn.receptance.weight, ffn.time_maa_r, ACT_SIGMOID)],
                                     x, block.ln2, state.ffn_x[lid])
        (x2,) = gemv_gated([(ffn.value.weight, kk, x, rr, ACT_NONE)], B, dev, copy=(h2, state.ffn_x[lid]))
    else:
        xk2, xr2 = ln_mix(x, block.ln2, state.ffn_x[lid], [ffn.time_maa_k, ffn.time_maa_r])
        kk, rr = gemv_multi([(ffn.key.weight, xk2, None, ACT_RELUSQ), (ffn.receptance.weight, xr2, None, ACT_SIGMOID)], B, dev)
        (x2,) = gemv_gated([(ffn.value.weight, kk, x, rr, ACT_NONE)], B, dev)                        # x + sigmoid(r) * value(relu(key)^2)
    return x2.view(B, 1, C)

