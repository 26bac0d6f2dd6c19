"""Generate tests/golden/v710_ref.pt by importing the reference's own VisualRWKV-v7/v7.10/src/model.py with the stand-ins of
make_golden_model.py (inert third-party packages, the repo's oracle as the CPU `wind_backstepping` op) and recording tensors only:
a 2-layer `RWKV` with the modality-routed Block (ln_v / ffn_v, src/model.py:233-262) at C = 128, T = 32, B = 2, run in bf16 (the
reference asserts bf16 at its WKV op), forward and backward, plus the end of one Block in fp32 (no WKV op involved).

The mask has an image block in the middle of row 0 and an image token at position 0 of row 1.

Size.  The model has 0.74 M parameters, 0.52 M of them in the eight channel-mix matrices; weights plus gradients would be 3 MB in bf16.  So
the matrices of BIG or more elements are not stored: their values come from tests/golden/det_weights.py by parameter name (full_state below,
which the test calls too), and of their gradients every ROW_STEP-th row is kept.  Everything smaller is recorded in full.

Run where /root/reference exists:   python tests/golden/make_golden_v710.py
"""
import os
import sys
from types import SimpleNamespace

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden.det_weights import det_tensor  # noqa: E402

REF = "/root/reference/VisualRWKV-v7/v7.10"
BIG, ROW_STEP, SEED = 4096, 4, 710


def full_state(small, shapes):
    """The model's fp32 state dict: the recorded tensors plus, for every matrix of BIG or more elements, det_tensor(name)."""
    return {k: (small[k].clone() if k in small else det_tensor(k, s, SEED)) for k, s in shapes.items()}


def keep_grad(g):
    return g[::ROW_STEP].clone() if g.numel() >= BIG else g.clone()


def main():
    from tests.golden import make_golden_model as base
    sys.path[:] = [p for p in sys.path if p != base.REF]
    sys.path.insert(0, REF)
    _lib = base.install_stubs()
    from src import model as ref            # the reference module itself (v7.10)
    g = torch.Generator().manual_seed(710)
    args = SimpleNamespace(n_embd=128, n_layer=2, dim_att=128, head_size_a=64, head_size_divisor=8, vocab_size=512,
                           dropout=0, grad_cp=0, ctx_len=64, load_model="", num_token_per_image=16, proj_type="mlp", patch_size=14)
    torch.manual_seed(4321)
    lm = ref.RWKV(args)
    base.randomize(lm, g)
    with torch.no_grad():
        for blk in lm.blocks:
            blk.att.r_k.copy_(torch.randn(blk.att.r_k.shape, generator=g) * 0.1)
            for ln in (blk.ln2, blk.ln_v):                  # the two experts' LayerNorms must differ for the routing to show
                ln.weight.copy_(1.0 + 0.3 * torch.randn(ln.weight.shape, generator=g))
                ln.bias.copy_(0.2 * torch.randn(ln.bias.shape, generator=g))
    shapes = {k: tuple(v.shape) for k, v in lm.state_dict().items()}
    small = {k: v.clone() for k, v in lm.state_dict().items() if v.numel() < BIG}
    lm.load_state_dict(full_state(small, shapes))
    out = {"args": vars(args), "state_small_fp32": small, "shapes": shapes}

    B, T = 2, 32
    mask = torch.zeros(B, T, 1, dtype=torch.bool)
    mask[0, 9:21] = True
    mask[1, 0] = True
    x32 = torch.randn(B, T, 128, generator=g) * 0.5

    # the end of Block 1 in fp32: x + where(mask, ffn_v(ln_v(x)), ffn(ln2(x)))
    with torch.no_grad():
        blk = lm.blocks[1]
        out["tail_fp32"] = {"x": x32.clone(), "y": x32 + torch.where(mask, blk.ffn_v(blk.ln_v(x32)), blk.ffn(blk.ln2(x32)))}

    lm = lm.bfloat16()
    x = x32.bfloat16().requires_grad_(True)
    logits = lm(x, mask)
    gout = (torch.randn(logits.shape, generator=g) * 0.1).bfloat16()
    logits.backward(gout)
    out["lm"] = {"x": x.detach().clone(), "mask": mask, "logits": logits.detach().clone(), "gout": gout, "dx": x.grad.clone(),
                 "grads": {n: keep_grad(p.grad) for n, p in lm.named_parameters() if n != "emb.weight"}}
    path = os.path.join(HERE, "v710_ref.pt")
    torch.save(out, path)
    print("wrote v710_ref.pt", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
