"""args.modality_ffn on the eager CPU path: the Block of VisualRWKV-v7/v7.10 (ln_v / ffn_v for image tokens, the layer ends in
x + where(mask, ffn_v(ln_v(x)), ffn(ln2(x)))) against a fixture recorded from the reference's own src/model.py
(tests/golden/make_golden_v710.py), and the properties of the mask.

Limits, by value from the tests of the v7.00 model: 1e-6 rel-RMS for an fp32 piece without the WKV op (tests/test_model_cpu.py); for the
bf16 run TOL = 1e-2 on the logits, 2 TOL on dx, 3 TOL on parameter gradients (tests/test_model_gpu.py, which holds the same kind of bf16
fixture to them)."""
import os
from types import SimpleNamespace

import pytest
import torch

from oracle.wkv7_oracle import rel_rms
from tests.golden.make_golden_v710 import BIG, ROW_STEP, full_state

GOLD = os.path.join(os.path.dirname(__file__), "golden", "v710_ref.pt")
TOL = 1e-2


@pytest.fixture(scope="module")
def gold():
    return torch.load(GOLD)


def lm_args(gold, **kw):
    d = dict(gold["args"], modality_ffn=1)
    d.update(kw)
    return SimpleNamespace(**d)


def lm(gold, **kw):
    from visualrwkv_amd.rwkv7 import RWKV
    m = RWKV(lm_args(gold, **kw))
    if kw.get("modality_ffn", 1):
        assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == gold["shapes"]      # the reference's keys, order and shapes
        m.load_state_dict(full_state(gold["state_small_fp32"], gold["shapes"]))
    return m


def test_state_dict_is_the_references(gold):
    from visualrwkv_amd.rwkv7 import RWKV
    mine = RWKV(lm_args(gold)).state_dict()
    assert list(mine.keys()) == list(gold["shapes"].keys())
    assert not any("ffn_v" in k or "ln_v" in k for k in RWKV(lm_args(gold, modality_ffn=0)).state_dict())
    blk = RWKV(lm_args(gold)).blocks[1]
    assert torch.equal(blk.ffn_v.x_k, blk.ffn.x_k) and float(blk.ffn_v.value.weight.detach().abs().sum()) == 0.0      # RWKV_CMix_x070's own initialisation
    assert torch.equal(blk.ln_v.weight, torch.ones(128)) and torch.equal(blk.ln_v.bias, torch.zeros(128))


def test_block_tail_fp32(gold):
    """x + where(mask, ffn_v(ln_v(x)), ffn(ln2(x))) in fp32 against the reference's modules."""
    m = lm(gold)
    g, blk = gold["tail_fp32"], m.blocks[1]
    mask = gold["lm"]["mask"]
    with torch.no_grad():
        x = g["x"]
        y = x + torch.where(mask, blk.ffn_v(blk.ln_v(x)), blk.ffn(blk.ln2(x)))
    assert rel_rms(y, g["y"]) < 1e-6
    wrong = x + torch.where(~mask, blk.ffn_v(blk.ln_v(x)), blk.ffn(blk.ln2(x)))
    assert rel_rms(wrong, g["y"]) > 1e-3              # the fixture tells the experts apart


def test_lm_forward_backward_matches_reference(gold):
    g = gold["lm"]
    m = lm(gold).bfloat16()
    x = g["x"].clone().requires_grad_(True)
    logits = m(x, mask=g["mask"])
    assert logits.shape == g["logits"].shape
    logits.backward(g["gout"])
    assert rel_rms(logits.detach().float(), g["logits"].float()) < TOL
    assert rel_rms(x.grad.float(), g["dx"].float()) < 2 * TOL
    named = dict(m.named_parameters())
    assert set(g["grads"]) == set(named) - {"emb.weight"}
    for n, ref in g["grads"].items():
        got = named[n].grad
        got = got[::ROW_STEP] if got.numel() >= BIG else got
        if float(ref.float().abs().max()) == 0.0:
            assert float(got.float().abs().max()) == 0.0, n
            continue
        assert rel_rms(got.float(), ref.float()) < 3 * TOL, n


def test_all_false_mask_is_the_model_without_ffn_v(gold):
    from visualrwkv_amd.rwkv7 import RWKV
    g = gold["lm"]
    m = lm(gold).bfloat16()
    plain = RWKV(lm_args(gold, modality_ffn=0))
    res = plain.load_state_dict(m.state_dict(), strict=False)
    assert not res.missing_keys and all(".ffn_v." in k or ".ln_v." in k for k in res.unexpected_keys)
    plain = plain.bfloat16()
    with torch.no_grad():
        a = m(g["x"], mask=torch.zeros_like(g["mask"]))
        b = plain(g["x"])
    assert torch.equal(a, b)


def test_all_true_mask_ignores_ffn_and_ln2(gold):
    g = gold["lm"]
    m = lm(gold).bfloat16()
    m(g["x"], mask=torch.ones_like(g["mask"])).backward(g["gout"])
    for n, p in m.named_parameters():
        if ".ffn." in n or ".ln2." in n:
            assert p.grad is None or not bool(p.grad.any()), n
        elif ".ffn_v." in n or ".ln_v." in n:
            assert p.grad is not None and bool(p.grad.any()), n


def test_mask_is_required_and_checked(gold):
    m = lm(gold).bfloat16()
    g = gold["lm"]
    with pytest.raises(ValueError):
        m(g["x"])
    with pytest.raises(ValueError):
        m(g["x"], mask=g["mask"][:, :, 0])
    from visualrwkv_amd.rwkv7 import RWKV
    with pytest.raises(ValueError):
        RWKV(lm_args(gold, modality_ffn=0)).bfloat16()(g["x"], mask=g["mask"])
    with pytest.raises(NotImplementedError):
        m.forward_stateful(g["x"])


def test_left_pad_extends_the_mask_with_false(gold):
    """T = 27 is padded to 32 on the left: the result is that of the 27 tokens with the mask moved along, whatever sits in the pad."""
    g = gold["lm"]
    m = lm(gold).bfloat16()
    x, mask = g["x"][:, :27], g["mask"][:, :27]
    with torch.no_grad():
        a = m(x, mask=mask)
        pad = m.pad_left(x, 5)
        b = m(pad, mask=torch.cat((torch.zeros_like(mask[:, :5]), mask), dim=1))[:, 5:]
    assert a.shape == (2, 27, gold["args"]["vocab_size"]) and torch.equal(a, b)


def _visual(gold, **kw):
    from visualrwkv_amd.visual import VisualRWKV
    args = lm_args(gold, vocab_size=65536, vision_towers=("dino",), vision_image_size=28, num_token_per_image=4, weight_decay=0.0,
                   vision_tower_kwargs={"dino": dict(depth=1, dim=32, heads=1)}, **kw)
    torch.manual_seed(0)
    return VisualRWKV(args)


def test_enable_pretrain_mode_trains_exactly_the_image_experts(gold):
    m = _visual(gold)
    m.enable_pretrain_mode()
    for n, p in m.rwkv.named_parameters():
        assert p.requires_grad == (".ffn_v." in n or ".ln_v." in n), n
    assert sum(p.requires_grad for p in m.rwkv.parameters()) == 2 * (2 + 3)      # per layer: ln_v weight, bias; ffn_v x_k, key, value
    with pytest.raises(ValueError):
        _visual(gold, modality_ffn=0).enable_pretrain_mode()


def test_visual_model_passes_the_mask_on(gold, tmp_path):
    from visualrwkv_amd.rwkv7 import IMAGE_TOKEN_INDEX
    m = _visual(gold)
    ids = torch.randint(0, 1000, (2, 16), generator=torch.Generator().manual_seed(3))
    ids[0, 3:7] = IMAGE_TOKEN_INDEX
    ids[1, 0:4] = IMAGE_TOKEN_INDEX
    batch = {"input_ids": ids, "labels": ids.clone(), "images": {"dino": torch.randn(2, 3, 28, 28)}}
    x, labels, mask = m.preparing_embedding(batch)
    assert mask.shape == (2, 16, 1) and mask.dtype == torch.bool and torch.equal(mask[..., 0], ids == IMAGE_TOKEN_INDEX)
    assert len(_visual(gold, modality_ffn=0).preparing_embedding(batch)) == 2          # without the flag nothing changes
    seen = []
    orig = m.rwkv.forward_features
    m.rwkv.forward_features = lambda x, layout=None, carry=None, mask=None, n_image=None: (seen.append(mask), orig(x, layout, carry, mask, n_image))[1]
    with torch.no_grad():
        for blk in m.rwkv.blocks:
            blk.ffn_v.value.weight.normal_(0, 0.05)
    loss = m.training_step(batch)
    loss.backward()
    assert torch.equal(seen[-1], mask) and m.rwkv.blocks[1].ffn_v.key.weight.grad is not None
    with torch.no_grad():
        m.generate(ids[:1, :8], {"dino": batch["images"]["dino"][:1]}, False, 1.0, 1.0, 3, -1)
    assert [s.shape[1] for s in seen[-3:]] == [8, 9, 10] and not bool(seen[-1][0, 8:].any()) and torch.equal(seen[-1][0, :8], mask[0, :8])
    with pytest.raises(NotImplementedError, match="re-normed per expert"):
        m.generate_stateful(ids[:1, :8], {"dino": batch["images"]["dino"][:1]}, False, 1.0, 1.0, 3, -1)
    with pytest.raises(NotImplementedError):
        m.train_step_cut(batch, 16)
    # a v7.00 checkpoint loads non-strictly; a foreign key is still an error
    sd = {k: v for k, v in m.rwkv.state_dict().items() if ".ffn_v." not in k and ".ln_v." not in k}
    torch.save(sd, tmp_path / "v700.pth")
    m.from_pretrained(str(tmp_path / "v700.pth"))
    sd["blocks.0.nope"] = torch.zeros(1)
    torch.save(sd, tmp_path / "bad.pth")
    with pytest.raises(RuntimeError):
        m.from_pretrained(str(tmp_path / "bad.pth"))


def test_route_plan_orders_image_rows_first_and_checks_a_passed_count():
    from visualrwkv_amd.fused import RoutePlan
    mask = torch.zeros(2, 8, 1, dtype=torch.bool)
    mask[0, 2:5] = True
    mask[1, 0] = True
    p = RoutePlan(mask, 4)
    assert p.n_v == 4 and p.ntok == 16 and not p.uniform and p.sel.tolist() == mask.view(-1).int().tolist()
    assert p.inv.tolist() == [2, 3, 4, 8, 0, 1, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15]
    assert torch.equal(p.pos[p.inv.long()], torch.arange(16, dtype=torch.int32)) and RoutePlan(mask).n_v == 4
    with pytest.raises(ValueError, match="holds 4 image tokens"):
        RoutePlan(mask, 5)
    assert RoutePlan(torch.zeros(1, 4, dtype=torch.bool)).uniform and RoutePlan(torch.ones(1, 4, 1, dtype=torch.bool)).uniform


def test_device_prefetcher_counts_the_image_tokens_on_the_host():
    from visualrwkv_amd import data
    ids = torch.randint(0, 1000, (2, 8))
    ids[0, 1:4] = data.IMAGE_TOKEN_INDEX
    out = data.DevicePrefetcher([], "cpu")._to_device({"input_ids": ids, "labels": ids.clone(), "sample_id": ["a", "b"]})
    assert out["n_image_tokens"] == 3
