"""Generate tests/golden/v6xx_ref.pt by importing the reference's own v6.xx Python (VisualRWKV-v6/v6.xx/src/model.py: RWKV_Tmix_x060_state,
Block, VisualRWKV.preparing_embedding / unidirectional_forward / training_step -- the "image as a per-layer WKV state" model) in this
container and recording tensors only.

Stand-ins, as for the other fixtures: `pytorch_lightning` and `src.dataset` are inert modules (deepspeed is absent and grad_cp = 0 never
asks for it); `fla.ops.rwkv6.fused_recurrent_rwkv6`, which RUN_CUDA_RWKV6_STATE calls (model.py:35-42), is the reference's OWN pure-PyTorch
statement of the same function, `naive_recurrent_rwkv6_fla` (VisualRWKV-v6/v6.xx/test_kernel.py:175-207), extracted from its file at
generation time and executed unmodified, as make_golden_wkv6.py does.  `einops` and `transformers` are the installed packages.

The run: 2 layers, C = 128 (2 heads), dim_ffn = 256, vocab 300, a tiny CLIPVisionModel (28 x 28 image, patch 7, grid_size 2 -> 4 pooled rows
+ CLS = 5 image rows), 3 samples of 24 ids -- the image token at position 5, at position 0 and absent -- in bf16 (the v6.0 fixture's
precision), forward and backward.

Size, as make_golden_v710.py: matrices of BIG or more elements are not stored; their values come from tests/golden/det_weights.py by
parameter name (full_state below, which the test calls too), and of the head's gradient every ROW_STEP-th row is kept.

Run where /root/reference exists:   python tests/golden/make_golden_v6xx.py
"""
import os
import sys
import types
from types import SimpleNamespace

import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from tests.golden.det_weights import det_tensor  # noqa: E402

REF = "/root/reference/VisualRWKV-v6/v6.xx"
BIG, ROW_STEP, SEED = 4096, 4, 62
ARGS = dict(n_embd=128, dim_att=128, n_layer=2, head_size_a=64, head_size_divisor=8, dim_ffn=256, vocab_size=300, dropout=0, grad_cp=0,
            ctx_len=40, load_model="", vision_tower_name="tiny", grid_size=2)
CLIP = dict(hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=2, image_size=28, patch_size=7)


def full_state(small, shapes):
    """The model's fp32 state dict: the recorded tensors plus, for every matrix of BIG or more elements, det_tensor(name)."""
    return {k: (small[k].clone() if k in small else det_tensor(k, s, SEED)) for k, s in shapes.items()}


def install_stubs():
    from make_golden_wkv6 import REF_TEST, extract_functions
    ns = {"torch": torch, "Optional": __import__("typing").Optional}
    exec(compile(extract_functions(REF_TEST, ["naive_recurrent_rwkv6_fla"])["naive_recurrent_rwkv6_fla"], REF_TEST, "exec"), ns)
    naive = ns["naive_recurrent_rwkv6_fla"]
    pl = types.ModuleType("pytorch_lightning")
    pl.LightningModule = nn.Module
    pl.__version__ = "1.9.5"
    plu = types.ModuleType("pytorch_lightning.utilities")
    plu.rank_zero_info = lambda *a, **k: None
    plu.rank_zero_only = lambda f: f
    pls = types.ModuleType("pytorch_lightning.strategies")
    pls.DeepSpeedStrategy = type("DeepSpeedStrategy", (), {})
    ds = types.ModuleType("src.dataset")
    ds.IGNORE_INDEX, ds.IMAGE_TOKEN_INDEX = -100, -200
    fla, ops, r6 = types.ModuleType("fla"), types.ModuleType("fla.ops"), types.ModuleType("fla.ops.rwkv6")
    r6.fused_recurrent_rwkv6 = r6.chunk_rwkv6 = r6.native_recurrent_rwkv6 = naive
    sys.modules.update({"pytorch_lightning": pl, "pytorch_lightning.utilities": plu, "pytorch_lightning.strategies": pls,
                        "src.dataset": ds, "fla": fla, "fla.ops": ops, "fla.ops.rwkv6": r6})
    os.environ["RWKV_JIT_ON"] = "0"


def main():
    install_stubs()
    sys.path.insert(0, REF)
    from src import model as ref
    import transformers
    clip_cfg = transformers.CLIPVisionConfig(**CLIP)

    class TinyClip:
        @staticmethod
        def from_pretrained(name):
            torch.manual_seed(5)
            return transformers.CLIPVisionModel(clip_cfg)

    ref.CLIPVisionModel = TinyClip
    g = torch.Generator().manual_seed(62)
    args = SimpleNamespace(**ARGS)
    torch.manual_seed(6)
    vm = ref.VisualRWKV(args)
    with torch.no_grad():
        for blk in vm.rwkv.blocks:                              # LayerNorms away from (1, 0): ln0 on both streams must show
            for ln in [blk.ln1, blk.ln2] + ([blk.ln0] if blk.layer_id == 0 else []):
                ln.weight.copy_(1.0 + 0.2 * torch.randn(ln.weight.shape, generator=g))
                ln.bias.copy_(0.1 * torch.randn(ln.bias.shape, generator=g))
    shapes = {k: tuple(v.shape) for k, v in vm.state_dict().items()}
    small = {k: v.clone() for k, v in vm.state_dict().items() if v.numel() < BIG}
    vm.load_state_dict(full_state(small, shapes))
    out = {"args": dict(ARGS), "clip": dict(CLIP), "state_small_fp32": small, "shapes": shapes,
           "provenance": "VisualRWKV-v6/v6.xx/src/model.py executed; fla's fused_recurrent_rwkv6 = test_kernel.py:175-207 naive_recurrent_rwkv6_fla"}
    vb = vm.bfloat16()
    B, T, C, H = 2, 24, 128, 2

    # ---- RWKV_Tmix_x060_state (layer 1) from a random state, forward and backward through y and the returned state
    tmix = vb.rwkv.blocks[1].att
    x = (torch.randn(B, T, C, generator=g) * 0.7).bfloat16().requires_grad_(True)
    s0 = (torch.rand(B, H, 64, 64, generator=g) * 2 - 1).requires_grad_(True)
    y, st = tmix(x, s0)
    gy = torch.randn(y.shape, generator=g).bfloat16()
    gst = torch.randn(st.shape, generator=g) * 0.1
    torch.autograd.backward([y, st], [gy, gst])
    out["tmix"] = {"x": x.detach().clone(), "s0": s0.detach().clone(), "y": y.detach().clone(), "state": st.detach().clone(), "gy": gy, "gstate": gst,
                   "gx": x.grad.clone(), "gs0": s0.grad.clone(),
                   "grads": {k: p.grad.clone() for k, p in tmix.named_parameters() if k in ("time_faaaa", "time_decay", "time_maa_w")}}
    vb.zero_grad(set_to_none=True)

    # ---- Block 0 (ln0) over 5 rows from None, then over T rows from the state that pass ended in
    with torch.no_grad():
        blk = vb.rwkv.blocks[0]
        xe = (torch.randn(B, 5, C, generator=g) * 0.7).bfloat16()
        ye, se = blk(xe, None)
        yt, s2 = blk(x.detach(), se)
        out["block"] = {"x_emb": xe, "y_emb": ye.clone(), "state_emb": se.clone(), "y": yt.clone(), "state": s2.clone()}

    # ---- VisualRWKV: embedding assembly, unidirectional pass, loss
    ids = torch.randint(0, ARGS["vocab_size"], (3, 24), generator=g)
    ids[0, 5] = ref.IMAGE_TOKEN_INDEX                  # image in the middle
    ids[1, 0] = ref.IMAGE_TOKEN_INDEX                  # image first; sample 2 has no image
    labels = ids.clone()
    labels[:, :8] = ref.IGNORE_INDEX
    labels[ids == ref.IMAGE_TOKEN_INDEX] = ref.IGNORE_INDEX
    images = torch.randn(3, 1, 3, 28, 28, generator=g)
    samples = {"input_ids": ids, "labels": labels, "images": images.bfloat16()}
    with torch.no_grad():
        xt, tg, imf = vb.preparing_embedding(samples)
    loss = vb.training_step(samples, 0)
    loss.backward()
    with torch.no_grad():
        logits, _ = vb(samples)
    assert float(vb.proj.weight.grad.float().abs().max()) > 0
    out["visual"] = {"input_ids": ids, "labels": labels, "images": images, "embeds_bf16": xt.clone(), "targets": tg.clone(),
                     "image_features_bf16": imf.clone(), "logits_bf16": logits.clone(), "loss": torch.tensor(float(loss)),
                     "grad_proj": vb.proj.weight.grad.clone(), "grad_head_rows": vb.rwkv.head.weight.grad[::ROW_STEP].clone()}
    path = os.path.join(HERE, "v6xx_ref.pt")
    torch.save(out, path)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
