"""Generate tests/golden/vtc_ref.pt by importing the reference's own VisualRWKV-v7/v7.04/src/model.py with the stand-ins of
make_golden_model.py (inert third-party packages, the repo's oracle as the CPU `wind_backstepping` op) and recording tensors only:
a `VisualTokenCompressor` with n_vtc_layer = 3 (forward, reversed, forward; src/model.py:327-374) at C = 128, B = 2, 29 input tokens (left-padded
with 3 zero rows to 32), run in bf16 (the reference asserts bf16 at its WKV op): the output, dx for a drawn gout, every parameter gradient.  And
`VisualRWKV.compress_visual_tokens` (src/model.py:516-529) on the same input as N = 1 image of L = 29 tokens with num_token_per_image = 4, under
'pool' (AdaptiveAvgPool1d: 29 -> 4) and under 'step' ([:, ::7]: 5 tokens).

Size, as make_golden_v710.py: the matrices of BIG or more elements are not stored; their values come from tests/golden/det_weights.py by parameter
name (full_state below, which the test calls too), and of their gradients every ROW_STEP-th row is kept.  Everything smaller is recorded in full.

Run where /root/reference exists:   python tests/golden/make_golden_vtc.py
"""
import os
import sys
from types import SimpleNamespace

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden.det_weights import det_tensor  # noqa: E402

REF = "/root/reference/VisualRWKV-v7/v7.04"
BIG, ROW_STEP, SEED = 4096, 4, 704


def full_state(small, shapes):
    """The compressor's fp32 state dict: the recorded tensors plus, for every matrix of BIG or more elements, det_tensor(name)."""
    return {k: (small[k].clone() if k in small else det_tensor(k, s, SEED)) for k, s in shapes.items()}


def keep_grad(g):
    return g[::ROW_STEP].clone() if g.numel() >= BIG else g.clone()


def main():
    from tests.golden import make_golden_model as base
    sys.path[:] = [p for p in sys.path if p != base.REF]
    sys.path.insert(0, REF)
    _lib = base.install_stubs()
    from src import model as ref            # the reference module itself (v7.04)
    g = torch.Generator().manual_seed(704)
    args = SimpleNamespace(n_embd=128, n_layer=4, n_vtc_layer=3, dim_att=128, head_size_a=64, head_size_divisor=8, vocab_size=512,
                           dropout=0, grad_cp=0, ctx_len=64, load_model="", num_token_per_image=4, proj_type="mlp")
    torch.manual_seed(4704)
    vtc = ref.VisualTokenCompressor(args)
    base.randomize(vtc, g)
    with torch.no_grad():
        for blk in vtc.blocks:
            blk.att.r_k.copy_(torch.randn(blk.att.r_k.shape, generator=g) * 0.1)
        vtc.ln_out.weight.copy_(1.0 + 0.3 * torch.randn(vtc.ln_out.weight.shape, generator=g))
        vtc.ln_out.bias.copy_(0.2 * torch.randn(vtc.ln_out.bias.shape, generator=g))
    shapes = {k: tuple(v.shape) for k, v in vtc.state_dict().items()}
    small = {k: v.clone() for k, v in vtc.state_dict().items() if v.numel() < BIG}
    vtc.load_state_dict(full_state(small, shapes))
    out = {"args": vars(args), "state_small_fp32": small, "shapes": shapes, "keys": list(vtc.state_dict().keys())}

    B, L = 2, 29
    vtc = vtc.bfloat16()
    x = (torch.randn(B, L, 128, generator=g) * 0.5).bfloat16().requires_grad_(True)
    y = vtc(x)
    gout = (torch.randn(y.shape, generator=g) * 0.1).bfloat16()
    y.backward(gout)
    out["vtc"] = {"x": x.detach().clone(), "y": y.detach().clone(), "gout": gout, "dx": x.grad.clone(),
                  "grads": {n: keep_grad(p.grad) for n, p in vtc.named_parameters()}}

    holder = SimpleNamespace(vtc=vtc, args=args)
    with torch.no_grad():
        feats = x.detach().view(B, 1, L, 128)
        out["compress"] = {"pool": ref.VisualRWKV.compress_visual_tokens(holder, feats, "pool").clone(),
                           "step": ref.VisualRWKV.compress_visual_tokens(holder, feats, "step").clone()}
    path = os.path.join(HERE, "vtc_ref.pt")
    torch.save(out, path)
    print("wrote vtc_ref.pt", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
