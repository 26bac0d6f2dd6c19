"""The visual token compressor (args.n_vtc_layer; VisualRWKV-v7/v7.03 and v7.04) on the eager CPU path, against a fixture recorded from the
reference's own v7.04 src/model.py (tests/golden/make_golden_vtc.py): rwkv7.VisualTokenCompressor with three Blocks (forward, reversed, forward)
at C = 128, B = 2, 29 tokens (pad 3), and VisualRWKV.compress_visual_tokens under 'pool' and 'step'; then what the model does around it.

Limits, by value from tests/test_routed_cpu.py (the same kind of bf16 fixture): TOL = 1e-2 on the output, 2 TOL on dx, 3 TOL on parameter
gradients.  The negative control (Block 1 run forward instead of reversed) has to miss the fixture by more than 1e-3."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from oracle.wkv7_oracle import rel_rms
from tests.golden.make_golden_vtc import BIG, ROW_STEP, full_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden", "vtc_ref.pt")
TOL = 1e-2


@pytest.fixture(scope="module")
def gold():
    return torch.load(GOLD)


def vtc_of(gold, **kw):
    from visualrwkv_amd.rwkv7 import VisualTokenCompressor
    m = VisualTokenCompressor(SimpleNamespace(**dict(gold["args"], **kw)))
    m.load_state_dict(full_state(gold["state_small_fp32"], gold["shapes"]))
    return m


def test_state_dict_is_the_references(gold):
    from visualrwkv_amd.rwkv7 import VisualTokenCompressor
    sd = VisualTokenCompressor(SimpleNamespace(**gold["args"])).state_dict()
    assert list(sd.keys()) == gold["keys"]                                            # the reference's keys in its order
    assert {k: tuple(v.shape) for k, v in sd.items()} == gold["shapes"]
    assert "blocks.0.ln0.weight" in sd and "ln_out.bias" in sd and not any(".ln0." in k for k in sd if not k.startswith("blocks.0."))
    # plain v7.00 Blocks whatever the language model is built with
    sd2 = VisualTokenCompressor(SimpleNamespace(**dict(gold["args"], state_tune=1, modality_ffn=1))).state_dict()
    assert list(sd2.keys()) == gold["keys"]


def test_forward_backward_matches_reference(gold):
    g = gold["vtc"]
    m = vtc_of(gold).bfloat16()
    x = g["x"].clone().requires_grad_(True)
    y = m(x)
    assert y.shape == g["y"].shape == (2, 29, 128)
    y.backward(g["gout"])
    assert rel_rms(y.detach().float(), g["y"].float()) < TOL
    assert rel_rms(x.grad.float(), g["dx"].float()) < 2 * TOL
    named = dict(m.named_parameters())
    assert set(g["grads"]) == set(named)
    for n, ref in g["grads"].items():
        got = named[n].grad
        got = got[::ROW_STEP] if got.numel() >= BIG else got
        if float(ref.float().abs().max()) == 0.0:
            assert float(got.float().abs().max()) == 0.0, n
            continue
        assert rel_rms(got.float(), ref.float()) < 3 * TOL, n


def test_block_1_runs_reversed(gold):
    """Negative control: the same weights with Block 1 run forward miss the fixture."""
    g = gold["vtc"]
    m = vtc_of(gold).bfloat16()
    with torch.no_grad():
        x = m.pad_left(g["x"], 3)
        v_first = torch.empty_like(x)
        for block in m.blocks:
            x, v_first = block(x, v_first)
        wrong = m.unpad(m.ln_out(x), 3)
        right = m(g["x"])
    assert rel_rms(wrong.float(), g["y"].float()) > 1e-3
    assert rel_rms(right.float(), g["y"].float()) < TOL


def test_pad_rows_are_zero_rows_not_eos(gold):
    m = vtc_of(gold).bfloat16()
    x = m.pad_left(gold["vtc"]["x"], 3)
    assert x.shape == (2, 32, 128) and not bool(x[:, :3].any()) and torch.equal(x[:, 3:], gold["vtc"]["x"])
    assert m.pad_left(x, 0) is x and m.unpad(x, 0) is x
    with pytest.raises(NotImplementedError, match="packed rows"):
        m(gold["vtc"]["x"], layout=object())


def _holder(gold):
    from visualrwkv_amd.visual import VisualRWKV
    return SimpleNamespace(vtc=vtc_of(gold).bfloat16(), args=SimpleNamespace(**gold["args"])), VisualRWKV


@pytest.mark.parametrize("reduction", ["pool", "step"])
def test_compress_visual_tokens_matches_reference(gold, reduction):
    h, V = _holder(gold)
    ref = gold["compress"][reduction]
    with torch.no_grad():
        got = V.compress_visual_tokens(h, gold["vtc"]["x"].view(2, 1, 29, 128), reduction)
    assert got.shape == ref.shape == {"pool": (2, 4, 128), "step": (2, 5, 128)}[reduction]
    assert rel_rms(got.float(), ref.float()) < TOL
    if reduction == "pool":                     # the pool is F.adaptive_avg_pool1d over tokens of the compressor's own output
        with torch.no_grad():
            want = F.adaptive_avg_pool1d(h.vtc(gold["vtc"]["x"]).permute(0, 2, 1), 4).permute(0, 2, 1)
        assert torch.equal(got, want)


def test_compress_visual_tokens_refuses(gold):
    h, V = _holder(gold)
    x = gold["vtc"]["x"].view(2, 1, 29, 128)
    with pytest.raises(ValueError, match="reduction"):
        V.compress_visual_tokens(h, x, "mean")
    h.args.num_token_per_image = 30
    with pytest.raises(ValueError, match="only reduces"):
        V.compress_visual_tokens(h, x)
    with pytest.raises(ValueError, match="no compressor"):
        V.compress_visual_tokens(SimpleNamespace(args=h.args), x)


# ------------------------------------------------------------------------------------------------ the model around it
def _visual(seed=0, **kw):
    """A 2-layer C = 128 model with the tiny DINO tower: 42 x 42 images = 9 tokens each, compressed to 4."""
    from visualrwkv_amd.visual import VisualRWKV
    d = dict(n_embd=128, n_layer=2, dim_att=128, head_size_a=64, head_size_divisor=8, vocab_size=65536, dropout=0, grad_cp=0, ctx_len=64,
             load_model="", num_token_per_image=4, proj_type="mlp", vision_towers=("dino",), vision_image_size=42, weight_decay=0.0,
             vision_tower_kwargs={"dino": dict(depth=1, dim=32, heads=1)})
    d.update(kw)
    torch.manual_seed(seed)
    return VisualRWKV(SimpleNamespace(**d))


def _batch(n_images=2, rows=2, T=24, holes=(8, 4)):
    """rows samples of T tokens; sample r has holes[r] image placeholders."""
    from visualrwkv_amd.rwkv7 import IMAGE_TOKEN_INDEX
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, 1000, (rows, T), generator=g)
    for r in range(rows):
        ids[r, 2 + r:2 + r + holes[r]] = IMAGE_TOKEN_INDEX
    labels = ids.clone()
    labels[ids == IMAGE_TOKEN_INDEX] = -100
    return {"input_ids": ids, "labels": labels, "images": {"dino": torch.randn(n_images, 3, 42, 42, generator=g)}, "sample_id": ["a", "b"][:rows]}


def test_n_vtc_layer_0_is_the_model_without_it():
    a, b = _visual(), _visual(n_vtc_layer=0)
    assert not a.has_vtc and not b.has_vtc and not any(k.startswith("vtc.") for k in b.state_dict())
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa.keys()) == list(sb.keys()) and all(torch.equal(sa[k], sb[k]) for k in sa)
    batch = _batch(2, 2, holes=(4, 4))
    with torch.no_grad():
        xa, xb = a.preparing_embedding(batch)[0], b.preparing_embedding(batch)[0]
    assert torch.equal(xa, xb)
    with pytest.raises(ValueError, match="no compressor"):
        a.init_vtc_weights()


def test_model_gains_the_compressor_and_trains_it():
    m = _visual(n_vtc_layer=2)
    keys = list(m.state_dict().keys())
    first = {p: next(i for i, k in enumerate(keys) if k.startswith(p)) for p in ("rwkv.", "vit.", "proj.", "vtc.")}
    assert first["rwkv."] < first["vit."] < first["proj."] < first["vtc."]            # the reference's registration order
    assert "vtc.blocks.0.ln0.weight" in keys and "vtc.ln_out.weight" in keys and "vtc.blocks.1.att.v0" in keys
    with torch.no_grad():                                                            # the reference zero-initialises these: make the Blocks live
        for n, p in m.named_parameters():
            if float(p.abs().sum()) == 0.0:
                p.normal_(0, 0.02)
    batch = _batch(4, 2, holes=(8, 8))
    x, labels = m.preparing_embedding(batch)
    assert x.shape == (2, 24, 128)
    # the placeholders hold compress_visual_tokens' rows, in order
    with torch.no_grad():
        feats = m.encode_images(batch["images"])
        assert feats.shape == (4, 9, 128)                                            # every token of every image: no 2-D pool
        want = m.compress_visual_tokens(feats.view(2, 2, 9, 128))
    assert want.shape == (2, 8, 128)
    from visualrwkv_amd.rwkv7 import IMAGE_TOKEN_INDEX
    assert torch.allclose(x[batch["input_ids"] == IMAGE_TOKEN_INDEX], want.reshape(16, 128), atol=1e-6)
    m.training_step(batch).backward()
    for n, p in m.named_parameters():
        if n.startswith(("vtc.", "proj.")):
            assert p.grad is not None and bool(p.grad.any()), n
    # the helpers see the new parameters with no special case
    n_train = sum(p.numel() for g in m.optimizer_groups() for p in g["params"])
    assert n_train == sum(p.numel() for p in m.parameters() if p.requires_grad) and any(p is m.vtc.ln_out.weight for g in m.optimizer_groups() for p in g["params"])
    m.freeze_rwkv(2); m.freeze_emb(); m.freeze_proj()
    assert all(p.requires_grad for p in m.vtc.parameters()) and not any(p.requires_grad for p in m.rwkv.parameters())
    # generate runs the same preparing_embedding
    with torch.no_grad():
        toks, _, _ = m.generate(batch["input_ids"][:1], {"dino": batch["images"]["dino"][:2]}, False, 1.0, 1.0, 2, -1)
    assert len(toks) == 2


def test_fewer_placeholders_than_features_truncates():
    m = _visual(n_vtc_layer=1)
    batch = _batch(4, 2, holes=(8, 4))           # 16 features, 12 placeholders
    with pytest.warns(UserWarning, match="image tokens: 12, but image features: 16"):
        x, _ = m.preparing_embedding(batch)
    with torch.no_grad():
        want = m.compress_visual_tokens(m.encode_images(batch["images"]).view(2, 2, 9, 128)).reshape(16, 128)[:12]
    from visualrwkv_amd.rwkv7 import IMAGE_TOKEN_INDEX
    assert torch.allclose(x[batch["input_ids"] == IMAGE_TOKEN_INDEX], want, atol=1e-6)


def test_init_vtc_weights_copies_exactly():
    m = _visual(n_vtc_layer=2)
    with torch.no_grad():
        for p in m.rwkv.parameters():
            p.add_(0.01 * torch.randn_like(p))
    m.init_vtc_weights()
    assert all(torch.equal(a, b) for a, b in zip(m.vtc.ln_out.state_dict().values(), m.rwkv.ln_out.state_dict().values()))
    for i in range(2):
        sv, sr = m.vtc.blocks[i].state_dict(), m.rwkv.blocks[i].state_dict()
        assert list(sv.keys()) == list(sr.keys()) and all(torch.equal(sv[k], sr[k]) for k in sv)
        assert all(a.data_ptr() != b.data_ptr() for a, b in zip(m.vtc.blocks[i].parameters(), m.rwkv.blocks[i].parameters()))     # copies, not ties


def test_error_cases():
    with pytest.raises(NotImplementedError, match="modality_ffn"):
        _visual(n_vtc_layer=1, modality_ffn=1)
    m = _visual(n_vtc_layer=1)
    with pytest.raises(ValueError, match="do not divide"):
        m.preparing_embedding(_batch(3, 2, holes=(4, 4)))
    with pytest.raises(NotImplementedError, match="train_step_cut"):
        m.train_step_cut(_batch(2, 2, T=32, holes=(4, 4)), 16)
    with pytest.raises(NotImplementedError, match="packed rows"):
        m.vtc(torch.zeros(1, 16, 128), layout=object())
    with pytest.raises(ValueError, match="only reduces"):
        _visual(n_vtc_layer=1, num_token_per_image=16).preparing_embedding(_batch(2, 2, holes=(16, 16)))


def test_engine_lays_the_compressor_out_with_the_projector():
    """dp.Zero1Engine orders its flat buffer by when the backward produces a gradient: `vtc.*` feeds the language model's input like `proj.*`, so
    inside each weight-decay class it comes after every language-model Block and before `proj.*`."""
    from visualrwkv_amd.dp import Zero1Engine
    m = _visual(n_vtc_layer=2)
    eng = Zero1Engine(m, lr=1e-3, bucket_mb=0.05)
    names = {id(p): n for n, p in m.named_parameters()}
    order = [names[id(p)] for p in eng.params]
    nwd = sum(1 for p in eng.params if len(p.squeeze().shape) >= 2)
    for part in (order[:nwd], order[nwd:]):
        kinds = ["late" if n.startswith(("vtc.", "proj.", "rwkv.emb.")) else "lm" for n in part]
        assert "late" in kinds and kinds == sorted(kinds, key=lambda k: k == "late"), part
        late = [n for n in part if n.startswith(("vtc.", "proj."))]
        assert [n.split(".")[0] for n in late] == sorted((n.split(".")[0] for n in late), reverse=True), late      # vtc before proj
    eng.close()


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from visualrwkv_amd.dp import Zero1Engine
    m = _live_model()
    batch = _batch(4, 2, holes=(8, 8))
    mine = {"input_ids": batch["input_ids"][rank:rank + 1], "labels": batch["labels"][rank:rank + 1],
            "images": {"dino": batch["images"]["dino"][2 * rank:2 * rank + 2]}, "sample_id": batch["sample_id"][rank:rank + 1]}
    eng = Zero1Engine(m, lr=0.0, weight_decay=0.0, grad_clip=0.0, bucket_mb=0.05)
    eng.zero_grad()
    m.training_step(mine).backward()
    eng.step(lr=0.0)
    torch.save({n: p.grad.detach().clone() / world for n, p in m.named_parameters() if n.startswith("vtc.")}, os.path.join(out_dir, f"r{rank}.pt"))
    dist.destroy_process_group()


def _live_model():
    m = _visual(n_vtc_layer=2)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in m.parameters():
            if float(p.abs().sum()) == 0.0:
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    return m


def test_world2_gloo_gives_the_compressor_the_single_process_gradients(tmp_path):
    """One sample (two images) per rank against both samples in one process: the loss is a batch mean, so the ranks' summed gradients over the
    world size are the single-process gradients.  fp32 on the CPU; takes a few seconds."""
    port = 31500 + os.getpid() % 2000
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = torch.load(tmp_path / "r0.pt"), torch.load(tmp_path / "r1.pt")
    m = _live_model()
    m.training_step(_batch(4, 2, holes=(8, 8))).backward()
    named = dict(m.named_parameters())
    assert set(r0) == {n for n in named if n.startswith("vtc.")} and len(r0) > 40
    for n, g in r0.items():
        assert torch.equal(g, r1[n]), n                     # the ranks hold the same reduced gradient
        ref = named[n].grad
        assert float(ref.abs().max()) > 0, n
        assert rel_rms(g, ref) < 1e-5, (n, rel_rms(g, ref))
