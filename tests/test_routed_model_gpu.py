"""args.modality_ffn at the model level on the MI355X: training_step of the 2-layer C = 2048 VisualRWKV of tests/test_packed_model_gpu.py with
`ln_v` / `ffn_v` in every Block, through the fused path -- fused.blocks_forward with a RoutePlan (the routed ln_mix kernels, the two channel
mixes on their own rows, the un-route gather) under its three memory modes, on ordinary and on packed rows, against the fp32 CPU evaluation of
the reference's `where` statement.  Bounds by value from tests/test_packed_model_gpu.py: the modes agree to 2e-3 on the loss and 4e-3 on
gradients; GPU against fp32 CPU 1e-2 on the loss, 2.6e-2 rel-RMS on every gradient group, scale error of the larger groups 8e-3."""
from types import SimpleNamespace

import pytest
import torch

from oracle.wkv7_oracle import rel_rms
from tests.parity import group_bias

pytestmark = pytest.mark.gpu

SEG_LENS = [[32, 32], [48, 16]]


def _visual(grad_cp, fused=True):
    from visualrwkv_amd.visual import VisualRWKV
    args = SimpleNamespace(n_embd=2048, n_layer=2, dim_att=2048, head_size_a=64, head_size_divisor=8, vocab_size=65536,
                           dropout=0, grad_cp=grad_cp, ctx_len=64, num_token_per_image=16, vision_towers=("dino",),
                           vision_image_size=56, load_model="", proj_type="mlp", weight_decay=0.0, fused=fused, modality_ffn=1,
                           check_image_tokens=not fused, vision_tower_kwargs={"dino": dict(depth=1, dim=64, heads=1)})
    torch.manual_seed(0)
    m = VisualRWKV(args)
    with torch.no_grad():
        for b in m.rwkv.blocks:
            b.att.output.weight.normal_(0, 0.02)
            b.ffn.value.weight.normal_(0, 0.02)
            b.ffn_v.value.weight.normal_(0, 0.02)
            b.ln_v.weight.normal_(1.0, 0.2)                  # the two experts must differ for a wrong route to show
            b.ln_v.bias.normal_(0, 0.2)
            b.ffn_v.x_k.uniform_(0, 1)
    m.freeze_emb()
    return m


def _batch(device, packed):
    """A LLaVA-like mask: 32 image tokens in the middle of row 0 (two images), 16 from position 0 of row 1 -- 48 of 128 tokens."""
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, 1000, (2, 64), generator=g)
    ids[0, 18:50] = 65535
    ids[1, 0:16] = 65535
    labels = ids.clone()
    labels[ids == 65535] = -100
    labels[:, :4] = -100
    imgs = {"dino": torch.randn(3, 3, 56, 56, generator=g).bfloat16()}
    batch = {"input_ids": ids.to(device), "labels": labels.to(device), "sample_id": ["0", "1"], "images": {k: v.to(device) for k, v in imgs.items()},
             "n_image_tokens": int((ids == 65535).sum())}
    if packed:
        t = 0
        for r, row in enumerate(SEG_LENS):
            t = 0
            for n in row:
                labels[r, t:t + 4] = -100
                t += n
        batch.update(labels=labels.to(device), sample_id=[["0", "1"], ["2", "3"]], seg_lens=SEG_LENS, n_samples=4)
    return batch


def _step(m, batch):
    m.zero_grad(set_to_none=True)
    loss = m.training_step(batch)
    loss.backward()
    return float(loss.detach()), {n: p.grad.float().cpu() for n, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("packed", [False, True], ids=["plain", "packed"])
def test_routed_step_under_every_memory_mode_and_against_fp32_cpu(monkeypatch, packed):
    from visualrwkv_amd import fused
    m = _visual(0).bfloat16().cuda()
    batch = _batch("cuda", packed)
    n_v, ntok = batch["n_image_tokens"], 128
    seen, rows = [], []
    real_blocks, real_linear = fused.blocks_forward, fused.linear
    monkeypatch.setattr(fused, "blocks_forward", lambda rwkv, x, grad_cp=0, layout=None, carry=None, route=None: (
        seen.append((grad_cp, layout is not None, route.n_v if route is not None else None)), real_blocks(rwkv, x, grad_cp, layout, carry, route))[1])
    names = {id(mod): n for n, mod in m.rwkv.named_modules()}
    monkeypatch.setattr(fused, "linear", lambda module, x: (rows.append((names[id(module)], x.numel() // x.shape[-1])), real_linear(module, x))[1])
    res = {}
    for mode in (0, 1, 2):
        m.args.grad_cp = mode
        rows.clear()
        res[mode] = _step(m, batch)
        if mode == 0:       # every channel-mix GEMM of a layer sees its own expert's rows only, never both sets
            for i in range(2):
                got = {n: r for n, r in rows if n.startswith(f"blocks.{i}.ffn")}
                assert got == {f"blocks.{i}.ffn_v.key": n_v, f"blocks.{i}.ffn_v.value": n_v,
                               f"blocks.{i}.ffn.key": ntok - n_v, f"blocks.{i}.ffn.value": ntok - n_v}, got
    assert seen == [(0, packed, n_v), (1, packed, n_v), (2, packed, n_v)]
    for mode in (1, 2):
        assert abs(res[mode][0] - res[0][0]) < 2e-3 * abs(res[0][0]), (mode, res[mode][0], res[0][0])
        for n, gr in res[0][1].items():
            assert rel_rms(res[mode][1][n], gr) < 4e-3, (mode, n)
    ref = _visual(0, fused=False).float()
    cb = _batch("cpu", packed)
    cb["images"] = {k: v.float() for k, v in cb["images"].items()}
    loss_ref, gref = _step(ref, cb)
    print(f"[routed] model step ({'packed' if packed else 'plain'}): GPU loss {res[0][0]:.4f}, fp32 CPU loss {loss_ref:.4f}")
    assert abs(res[0][0] - loss_ref) < 1e-2 * abs(loss_ref), (res[0][0], loss_ref)
    checked, experts = 0, 0
    for n, gr in gref.items():
        if gr.abs().max() == 0 or gr.numel() < 64:
            continue
        e = rel_rms(res[0][1][n], gr)
        print(f"[routed] {n}: rel-RMS {e:.3e}")
        assert e < 2.6e-2, (n, e)
        if gr.numel() >= 1024:
            group_bias(res[0][1][n], gr, n, max_scale_err=8e-3)
        checked += 1
        experts += n.startswith("rwkv.") and (".ffn_v." in n or ".ln_v." in n or ".ffn." in n or ".ln2." in n)
    assert checked >= 30 and experts == 2 * 10          # per layer: ln2, ln_v (weight, bias), ffn, ffn_v (x_k, key, value)


def test_uniform_masks_launch_one_expert(monkeypatch):
    """No image token / image tokens only: one channel mix runs, on every row, and nothing is gathered."""
    from visualrwkv_amd import fused
    m = _visual(0).bfloat16().cuda()
    x = torch.randn(2, 32, 2048, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5)).bfloat16()
    rows, gathers = [], []
    real_linear, real_gather = fused.linear, fused.row_gather
    names = {id(mod): n for n, mod in m.rwkv.named_modules()}
    monkeypatch.setattr(fused, "linear", lambda module, x: (rows.append((names[id(module)], x.numel() // x.shape[-1])), real_linear(module, x))[1])
    monkeypatch.setattr(fused, "row_gather", lambda src, idx: (gathers.append(1), real_gather(src, idx))[1])
    for val, live, dead in ((False, ".ffn.", ".ffn_v."), (True, ".ffn_v.", ".ffn.")):
        rows.clear()
        xx = x.clone().requires_grad_(True)
        m.zero_grad(set_to_none=True)
        h, _ = m.rwkv(xx, hidden_only=True, mask=torch.full((2, 32, 1), val, device="cuda"))
        h.float().sum().backward()
        ff = [(n, r) for n, r in rows if ".ffn" in n]
        assert all(live in n and r == 64 for n, r in ff) and len(ff) == 4, ff
        for n, p in m.rwkv.named_parameters():
            if dead in n or (".ln2." if val else ".ln_v.") in n:
                assert p.grad is None or not bool(p.grad.any()), n
    assert not gathers


def test_pretrain_mode_step_trains_only_the_image_experts():
    m = _visual(0).bfloat16().cuda()
    m.enable_pretrain_mode()
    m.freeze_proj()
    _, grads = _step(m, _batch("cuda", False))
    assert grads and all(".ffn_v." in n or ".ln_v." in n for n in grads), sorted(grads)
    assert len(grads) == 2 * 5 and all(bool(g.any()) for g in grads.values())


def test_a_wrong_image_count_is_an_error_not_a_wrong_route():
    """n_image_tokens comes from the host (data.DevicePrefetcher); the plan checks it against the mask's own count by the first backward."""
    m = _visual(0).bfloat16().cuda()
    batch = _batch("cuda", False)
    batch["n_image_tokens"] += 16
    m.zero_grad(set_to_none=True)
    with pytest.raises(ValueError, match="wrong expert"):
        m.training_step(batch).backward()
