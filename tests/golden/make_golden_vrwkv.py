"""Generate tests/golden/vrwkv_ref.pt by importing the reference's own VisualRWKV-v7/v7.10/src/model.py with the stand-ins of
make_golden_model.py (inert third-party packages, the repo's oracle as the CPU `wind_backstepping` op), exactly as make_golden_v710.py does,
and recording tensors only:

  vrwkv   the reference's `VRWKV` (Conv2d patch embedding, its 6 VBlocks, ln_out, the ImageNet head) at n_embd = 128, patch_size = 16, 64 x 64
          images (16 tokens), B_img = 2, in bf16: features and logits, and the gradients for given upstream gradients of BOTH outputs.
  step    one `VisualRWKV.training_step` (v7.10: rwkv + vrwkv) with a 2-layer language model, 16 placeholders per sample and `cls_labels`:
          the loss and the gradient of vrwkv.emb.weight.  The encoder carries the weights of the first part (a VBlock initialised with
          layer_id >= n_layer = 2 holds infinities in the reference too; the state is loaded over it).

Size.  Matrices of BIG or more elements are not stored: their values come from tests/golden/det_weights.py by parameter name (full_state
below, which the test calls too).  Of the gradients of such matrices every ROW_STEP-th row is kept, and only for emb, head, and Block 0's
time mix and channel-mix key -- six Blocks' worth would be 0.7 MB; the gradients of every smaller tensor (LayerNorms, lerp vectors, LoRA biases, k_k / k_a / r_k of all six
Blocks, ln_out) are recorded in full, so every Block is covered.  The input images come from det_image by seed (images() below).

Run where /root/reference exists:   python tests/golden/make_golden_vrwkv.py
"""
import os
import sys
from types import SimpleNamespace

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden.det_weights import det_image, det_tensor  # noqa: E402

REF = "/root/reference/VisualRWKV-v7/v7.10"
BIG, ROW_STEP, SEED = 4096, 4, 7100
BIG_GRADS = ("emb.", "head.", "blocks.0.att.", "blocks.0.ffn.key.")          # whose matrices' gradient rows are kept
IMAGE_SEED = 7100


def images():
    """The two 64 x 64 input images (not stored: 49 KB)."""
    return (det_image((2, 3, 64, 64), IMAGE_SEED) * 0.5).bfloat16()


def full_state(small, shapes, prefix=""):
    """The fp32 state dict: the recorded tensors plus, for every matrix of BIG or more elements, det_tensor(prefix + name)."""
    return {k: (small[k].clone() if k in small else det_tensor(prefix + k, s, SEED)) for k, s in shapes.items()}


def keep_grad(name, g):
    if g.numel() < BIG:
        return g.clone()
    return g[::ROW_STEP].clone() if name.startswith(BIG_GRADS) else None


def main():
    from tests.golden import make_golden_model as base
    sys.path[:] = [p for p in sys.path if p != base.REF]
    sys.path.insert(0, REF)
    _lib = base.install_stubs()
    from src import model as ref            # the reference module itself (v7.10)
    g = torch.Generator().manual_seed(7100)
    common = dict(n_embd=128, dim_att=128, head_size_a=64, head_size_divisor=8, dropout=0, grad_cp=0, ctx_len=64, load_model="",
                  num_token_per_image=16, proj_type="mlp", patch_size=16, image_size=64)
    args = SimpleNamespace(n_layer=6, vocab_size=512, **common)
    torch.manual_seed(47100)
    vr = ref.VRWKV(args)
    base.randomize(vr, g)
    with torch.no_grad():
        for blk in vr.blocks:
            blk.att.r_k.copy_(torch.randn(blk.att.r_k.shape, generator=g) * 0.1)
        vr.ln_out.weight.copy_(1.0 + 0.3 * torch.randn(vr.ln_out.weight.shape, generator=g))
        vr.ln_out.bias.copy_(0.2 * torch.randn(vr.ln_out.bias.shape, generator=g))
    shapes = {k: tuple(v.shape) for k, v in vr.state_dict().items()}
    small = {k: v.clone() for k, v in vr.state_dict().items() if v.numel() < BIG}
    vr.load_state_dict(full_state(small, shapes, "vrwkv."))
    out = {"args": dict(vars(args), n_vrwkv_layer=6), "state_small_fp32": small, "shapes": shapes, "keys": list(vr.state_dict().keys())}

    vr = vr.bfloat16()
    imgs = images()
    feats, logits = vr(imgs)
    gf = (torch.randn(feats.shape, generator=g) * 0.1).bfloat16()
    gl = (torch.randn(logits.shape, generator=g) * 0.1).bfloat16()
    torch.autograd.backward([feats, logits], [gf, gl])
    grads = {n: keep_grad(n, p.grad) for n, p in vr.named_parameters()}
    out["vrwkv"] = {"features": feats.detach().clone(), "logits": logits.detach().clone(), "g_features": gf, "g_logits": gl,
                    "grads": {n: v for n, v in grads.items() if v is not None}}

    # one training step of the whole v7.10 model: 2-layer language model with ln_v / ffn_v, the encoder above
    args2 = SimpleNamespace(n_layer=2, vocab_size=65536, **common)
    torch.manual_seed(47101)
    full = ref.VisualRWKV(args2)
    base.randomize(full.rwkv, g)
    lm_shapes = {k: tuple(v.shape) for k, v in full.rwkv.state_dict().items()}
    lm_small = {k: v.clone() for k, v in full.rwkv.state_dict().items() if v.numel() < BIG}
    full.rwkv.load_state_dict(full_state(lm_small, lm_shapes, "rwkv."))
    full.vrwkv.load_state_dict(full_state(small, shapes, "vrwkv."))
    full = full.bfloat16()
    B, T = 2, 32
    ids = torch.randint(0, 1000, (B, T), generator=g)
    ids[0, 3:19] = 65535
    ids[1, 0:16] = 65535
    labels = ids.clone()
    labels[ids == 65535] = -100
    batch = {"input_ids": ids, "labels": labels, "images": {"image": imgs, "num_image_per_sample": [1, 1]}, "sample_id": ["a", "b"],
             "cls_labels": torch.tensor([17, 901])}
    loss = full.training_step(batch, 0)
    loss.backward()
    out["step"] = {"args": dict(vars(args2), n_vrwkv_layer=6, modality_ffn=1), "lm_state_small_fp32": lm_small, "lm_shapes": lm_shapes,
                   "input_ids": ids, "labels": labels, "cls_labels": batch["cls_labels"], "loss": loss.detach().float().clone(),
                   "d_emb_weight": full.vrwkv.emb.weight.grad[::ROW_STEP].clone()}
    path = os.path.join(HERE, "vrwkv_ref.pt")
    torch.save(out, path)
    print("wrote vrwkv_ref.pt", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
