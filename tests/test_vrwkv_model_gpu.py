"""args.n_vrwkv_layer at the model level on the MI355X: training_step of a 2-layer VisualRWKV whose images come from a 2-Block RWKV vision encoder
(v7.10's `vrwkv`), through the fused path -- the patch-embedding kernel with its weight-gradient kernel (vrwkv_patch_embed_wgrad_bf16), the Blocks
through _block_segment, and the tail kernels (ln_out + scatter into the placeholder rows + the mean over tokens for the ImageNet head) -- under its
three memory modes, against the eager modules (nn.Conv2d, nn.LayerNorm, mean, masked_scatter) in fp32 on the CPU, with and without the image experts
(args.modality_ffn) and with `cls_labels` in the batch.

n_embd = 256, so that the weight-gradient kernel is the one that runs (asserted through fused.patch_wgrad_supported); 128 x 128 images = 64 tokens,
one image per sample, two samples of 96 tokens.  Row 0 holds 64 placeholders; row 1 holds 64 (`full`) or 48 (`short`: the last 16 features get row
-1 and are dropped in both directions -- but still count in the head's mean -- where the eager path truncates and warns).

Bounds by value from tests/test_vtc_model_gpu.py: the modes agree to 2e-3 on the loss and 4e-3 on gradients; GPU against fp32 CPU 1e-2 on the loss,
2.6e-2 rel-RMS on every gradient group, scale error of the larger groups 8e-3."""
import copy
import warnings
from types import SimpleNamespace

import pytest
import torch

from oracle.wkv7_oracle import rel_rms
from tests.parity import group_bias

pytestmark = pytest.mark.gpu

IMG, L_IMG, C, T = 128, 64, 256, 96


def _visual(modality, fused=True):
    from visualrwkv_amd.visual import VisualRWKV
    args = SimpleNamespace(n_embd=C, n_layer=2, n_vrwkv_layer=2, modality_ffn=modality, dim_att=C, head_size_a=64, head_size_divisor=8, vocab_size=65536,
                           dropout=0, grad_cp=0, ctx_len=T, num_token_per_image=L_IMG, image_size=IMG, patch_size=16, load_model="", proj_type="mlp",
                           weight_decay=0.0, fused=fused, check_image_tokens=not fused)
    torch.manual_seed(0)
    m = VisualRWKV(args)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for blocks in (m.rwkv.blocks, m.vrwkv.blocks):
            for b in blocks:
                b.att.output.weight.copy_(torch.randn(b.att.output.weight.shape, generator=g) * 0.02)
                b.ffn.value.weight.copy_(torch.randn(b.ffn.value.weight.shape, generator=g) * 0.02)
                if getattr(b, "ffn_v", None) is not None:
                    b.ffn_v.value.weight.copy_(torch.randn(b.ffn_v.value.weight.shape, generator=g) * 0.02)
        m.vrwkv.ln_out.weight.copy_(1.0 + 0.2 * torch.randn(C, generator=g))         # a wrong ln_out would otherwise look like none
        m.vrwkv.ln_out.bias.copy_(0.2 * torch.randn(C, generator=g))
    m.freeze_emb()
    return m


@pytest.fixture(scope="module", params=[0, 1], ids=["plain", "modality_ffn"])
def models(request):
    """(the bf16 model on the GPU with args.fused, its fp32 twin on the CPU without), built once per variant and never stepped."""
    cpu = _visual(request.param, fused=False).float()
    gpu = copy.deepcopy(cpu)
    for mod in gpu.modules():                    # every module holds the argument object it was built from (the encoder's Blocks a copy)
        if isinstance(getattr(mod, "args", None), SimpleNamespace):
            mod.args.fused, mod.args.check_image_tokens = True, False
    return gpu.bfloat16().cuda(), cpu


def _batch(device, holes):
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, 1000, (2, T), generator=g)
    ids[0, 18:18 + holes[0]] = 65535
    ids[1, 0:holes[1]] = 65535
    labels = ids.clone()
    labels[ids == 65535] = -100
    labels[:, :4] = -100
    imgs = (torch.randn(2, 3, IMG, IMG, generator=g) * 0.5).bfloat16()
    return {"input_ids": ids.to(device), "labels": labels.to(device), "sample_id": ["0", "1"], "images": {"image": imgs.to(device), "num_image_per_sample": [1, 1]},
            "cls_labels": torch.tensor([3, 977], device=device)}


def _step(m, batch):
    m.zero_grad(set_to_none=True)
    loss = m.training_step(batch)
    loss.backward()
    return float(loss.detach()), {n: p.grad.float().cpu() for n, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("case,holes", [("full", (64, 64)), ("short", (64, 48))])
def test_vrwkv_step_under_every_memory_mode_and_against_fp32_cpu(monkeypatch, models, case, holes):
    from visualrwkv_amd import fused
    m, ref = models
    assert m.args.fused and m.vrwkv.blocks[1].att.args.fused and not ref.args.fused
    batch = _batch("cuda", holes)
    assert fused.patch_wgrad_supported(batch["images"]["image"], m.vrwkv.emb.weight) and fused.PATCH_WGRAD and fused.VRWKV_TAIL
    tails, wgrads = [], []
    real_tail, real_bwd = fused.ln_scatter_mean, fused._PatchEmbedTrain.backward
    monkeypatch.setattr(fused, "ln_scatter_mean", lambda x, delta, ln, e=None, r=None: (
        tails.append((tuple(x.shape), delta is None, int((r < 0).sum()))), real_tail(x, delta, ln, e, r))[1])
    monkeypatch.setattr(fused._PatchEmbedTrain, "backward", staticmethod(lambda ctx, dout: (wgrads.append(ctx.kernel), real_bwd(ctx, dout))[1]))
    # the text rows of the embedding keep their bits
    with torch.no_grad():
        x = m.preparing_embedding(batch)
        assert len(x) == 4 and (x[2] is None) == (not m.args.modality_ffn) and x[3].shape == (2, 1000)
        sel = batch["input_ids"] == 65535
        assert torch.equal(x[0][~sel], m.rwkv.emb(batch["input_ids"])[~sel]) and bool(torch.isfinite(x[0].float()).all())
    tails.clear()
    res = {}
    for mode in (0, 1, 2):
        m.args.grad_cp = mode
        for blk in m.vrwkv.blocks:
            blk.args.grad_cp = mode
        m.vrwkv.args.grad_cp = mode
        res[mode] = _step(m, batch)
    n_drop = 2 * L_IMG - sum(holes)
    assert tails == [((2, L_IMG, C), False, n_drop)] * 3, tails
    assert wgrads == [True] * 3, wgrads
    for mode in (1, 2):
        assert abs(res[mode][0] - res[0][0]) < 2e-3 * abs(res[0][0]), (mode, res[mode][0], res[0][0])
        for n, gr in res[0][1].items():
            assert rel_rms(res[mode][1][n], gr) < 4e-3, (mode, n)
    m.args.grad_cp = 0
    m.vrwkv.args.grad_cp = 0
    cb = _batch("cpu", holes)
    cb["images"]["image"] = cb["images"]["image"].float()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # `short`: the eager path warns that it truncates
        loss_ref, gref = _step(ref, cb)
    print(f"[vrwkv] model step ({case}): GPU loss {res[0][0]:.4f}, fp32 CPU loss {loss_ref:.4f}")
    assert abs(res[0][0] - loss_ref) < 1e-2 * abs(loss_ref), (res[0][0], loss_ref)
    assert set(gref) == set(res[0][1])
    for must in ("vrwkv.emb.weight", "vrwkv.emb.bias", "vrwkv.head.weight", "vrwkv.head.bias", "vrwkv.blocks.0.att.key.weight", "vrwkv.blocks.1.ffn.key.weight",
                 "vrwkv.ln_out.weight"):
        assert must in gref and float(gref[must].abs().max()) > 0, must
    checked, v_groups = 0, 0
    for n, gr in gref.items():
        if gr.abs().max() == 0 or gr.numel() < 64:
            continue
        e = rel_rms(res[0][1][n], gr)
        print(f"[vrwkv] {n}: rel-RMS {e:.3e}")
        assert e < 2.6e-2, (n, e)
        if gr.numel() >= 1024:
            group_bias(res[0][1][n], gr, n, max_scale_err=8e-3)
        checked += 1
        v_groups += n.startswith("vrwkv.")
    assert checked >= 60 and v_groups >= 30, (checked, v_groups)
    # the composite tail (VRWKV_TAIL=0: add_ln, index_copy, mean) gives the same loss
    monkeypatch.setattr(fused, "VRWKV_TAIL", False)
    loss_c, _ = _step(m, batch)
    assert len(tails) == 3 and abs(loss_c - res[0][0]) < 2e-3 * abs(res[0][0]) and abs(loss_c - loss_ref) < 1e-2 * abs(loss_ref), (loss_c, res[0][0], loss_ref)
