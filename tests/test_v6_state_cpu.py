"""The v6.xx "image as a per-layer WKV state" model on CPU: the host-side mirrors (RWKV_Tmix_x060.forward_state, Block.forward_state,
VisualRWKV6 with args.image_state = 1) around an oracle-backed stand-in for RUN_CUDA_RWKV6_STATE, against tests/golden/v6xx_ref.pt --
tensors recorded from the reference's own v6.xx Python (tests/golden/make_golden_v6xx.py).  Tolerances are the ones tests/test_v6_cpu.py
holds the v6.0 modules to (two bf16 pipelines): 1e-2 outputs, 2e-2 input gradients and logits, 3e-2 parameter gradients, 5e-2 for the
projector's and the head's, 2e-2 relative on the loss."""
import os
from types import SimpleNamespace

import pytest
import torch

from oracle.wkv6_oracle import wkv6_naive
from oracle.wkv7_oracle import rel_rms
from tests.golden.make_golden_v6xx import ROW_STEP, full_state

GOLD = os.path.join(os.path.dirname(__file__), "golden", "v6xx_ref.pt")


@pytest.fixture(scope="module")
def gold():
    return torch.load(GOLD)


def oracle_wkv_state(B, T, C, H, r, k, v, w, u, s):
    """RUN_CUDA_RWKV6_STATE's signature on the oracle recurrence (differentiable by autograd): s and the returned state are [key][value]."""
    f = lambda x: x.double().view(B, T, H, C // H)
    y, S = wkv6_naive(f(r), f(k), f(v), f(w), u.double(), state0=s.double().transpose(-1, -2) if s is not None else None)
    return y.reshape(B, T, C).to(r.dtype), S.transpose(-1, -2).float()


def _visual(gold, image_state=1):
    import transformers
    from visualrwkv_amd import visual6
    args = SimpleNamespace(**gold["args"], image_state=image_state)
    clip = transformers.CLIPVisionModel(transformers.CLIPVisionConfig(**gold["clip"]))
    m = visual6.VisualRWKV6(args, clip, clip.config.hidden_size)
    assert list(m.state_dict().keys()) == list(gold["shapes"].keys())          # the reference's keys: forward_state adds no parameter
    m.load_state_dict(full_state(gold["state_small_fp32"], gold["shapes"]))
    return m.bfloat16()


def _samples(gold):
    vis = gold["visual"]
    return {"input_ids": vis["input_ids"], "labels": vis["labels"], "images": vis["images"].bfloat16()}


def test_tmix_forward_state_against_reference(gold):
    t = gold["tmix"]
    tmix = _visual(gold).rwkv.blocks[1].att
    x = t["x"].clone().requires_grad_(True)
    s0 = t["s0"].clone().requires_grad_(True)
    y, st = tmix.forward_state(x, s0, oracle_wkv_state)
    torch.autograd.backward([y, st], [t["gy"], t["gstate"]])
    assert rel_rms(y.float(), t["y"].float()) < 1e-2
    assert rel_rms(st, t["state"]) < 1e-2
    assert rel_rms(x.grad.float(), t["gx"].float()) < 2e-2
    assert rel_rms(s0.grad, t["gs0"]) < 2e-2
    named = dict(tmix.named_parameters())
    for k, g in t["grads"].items():
        assert rel_rms(named[k].grad.float(), g.float()) < 3e-2, k


def test_block_forward_state_against_reference(gold):
    """Block 0 (ln0 on every call) over 5 image rows from None, then over the text rows from the state that pass ended in."""
    b = gold["block"]
    blk = _visual(gold).rwkv.blocks[0]
    with torch.no_grad():
        ye, se = blk.forward_state(b["x_emb"], None, oracle_wkv_state)
        yt, s2 = blk.forward_state(gold["tmix"]["x"], se, oracle_wkv_state)
    assert rel_rms(ye.float(), b["y_emb"].float()) < 1e-2 and rel_rms(se, b["state_emb"]) < 1e-2
    assert rel_rms(yt.float(), b["y"].float()) < 1e-2 and rel_rms(s2, b["state"]) < 1e-2


def test_preparing_embedding_state(gold):
    """Image in the middle (sample 0), image first (1), no image (2): the text is what stands right of the image token, the sample
    without an image keeps all its ids and gets zeroed features."""
    from visualrwkv_amd.visual6 import IGNORE_INDEX
    m, vis = _visual(gold), gold["visual"]
    with torch.no_grad():
        x, tg, feats = m.preparing_embedding_state(_samples(gold))
    assert torch.equal(tg, vis["targets"])
    assert x.shape == vis["embeds_bf16"].shape and rel_rms(x.float(), vis["embeds_bf16"].float()) < 1e-2
    assert rel_rms(feats.float(), vis["image_features_bf16"].float()) < 1e-2
    ids, lab = vis["input_ids"], vis["labels"]
    assert x.shape[1] == 24 and feats.shape[1] == 5
    assert torch.equal(tg[0, :18], lab[0, 6:]) and bool((tg[0, 18:] == IGNORE_INDEX).all()) and float(x[0, 18:].abs().max()) == 0.0
    assert torch.equal(tg[1, :23], lab[1, 1:]) and torch.equal(tg[2], lab[2])
    assert torch.equal(x[2], m.rwkv.emb(ids[2]))
    assert float(feats[2].abs().max()) == 0.0 and float(feats[0].abs().max()) > 0.0
    m.args.ctx_len = 10                                         # truncate_input: the beginning is kept when it carries a label
    with torch.no_grad():
        x2, tg2, _ = m.preparing_embedding_state(_samples(gold))
    assert x2.shape[1] == 10 and torch.equal(tg2, tg[:, :10]) and torch.equal(x2, x[:, :10])
    bad = _samples(gold)
    bad["input_ids"] = bad["input_ids"].clone()
    bad["input_ids"][0, 7] = -200
    with pytest.raises(ValueError):
        m.preparing_embedding_state(bad)


def test_unidirectional_forward_and_training_step(gold):
    m, vis = _visual(gold), gold["visual"]
    samples = _samples(gold)
    loss = m.training_step(samples, 0, oracle_wkv_state)
    loss.backward()
    assert abs(float(loss.detach()) - float(vis["loss"])) < 2e-2 * abs(float(vis["loss"]))
    with torch.no_grad():
        logits, _ = m(samples, oracle_wkv_state)
    assert rel_rms(logits.float(), vis["logits_bf16"].float()) < 2e-2
    assert float(vis["grad_proj"].float().abs().max()) > 0      # the projector is reached only through dL/dS
    assert rel_rms(m.proj.weight.grad.float(), vis["grad_proj"].float()) < 5e-2
    assert rel_rms(m.rwkv.head.weight.grad[::ROW_STEP].float(), vis["grad_head_rows"].float()) < 5e-2


def test_grad_cp_checkpoints_the_two_passes(gold):
    m = _visual(gold)
    samples = _samples(gold)
    m.training_step(samples, 0, oracle_wkv_state).backward()
    g0 = m.proj.weight.grad.clone()
    m.zero_grad()
    m.args.grad_cp = 1
    m.training_step(samples, 0, oracle_wkv_state).backward()
    assert torch.equal(m.proj.weight.grad, g0)


def test_image_state_0_is_unchanged(gold):
    """The default keeps the bidirectional model: same logits as a model whose args do not know the switch."""
    from tests.test_v6_cpu import _oracle_wkv
    m0, m1 = _visual(gold, image_state=0), _visual(gold, image_state=0)
    del m1.args.image_state
    samples = _samples(gold)
    with torch.no_grad():
        a, ta = m0(samples, _oracle_wkv())
        b, tb = m1(samples, _oracle_wkv())
    assert torch.equal(a, b) and torch.equal(ta, tb)
    assert a.shape[1] == 5 + 5 + 24                              # left pad to the latest image position | the image span in the context | the longest tail
    with pytest.raises(NotImplementedError):
        m0.generate(samples["input_ids"][:1], samples["images"][:1], False, 1.0, 1.0, 2, 0)


def test_generate_is_the_argmax_of_the_last_row(gold):
    m = _visual(gold)
    s = _samples(gold)
    ids, images = s["input_ids"][:1], s["images"][:1]
    with pytest.raises(NotImplementedError):
        m.generate(ids, images, True, 1.0, 1.0, 2, -1, wkv=oracle_wkv_state)
    out = m.generate(ids, images, False, 1.0, 1.0, 3, -1, wkv=oracle_wkv_state)
    assert len(out) == 3
    with torch.no_grad():
        cur = ids
        for tok in out:                                          # each token: unidirectional_forward on the ids so far
            x, _, feats = m.preparing_embedding_state({"input_ids": cur, "images": images, "labels": torch.full_like(cur, -100)}, truncate=False)
            assert int(m.unidirectional_forward(x, feats, oracle_wkv_state)[0, -1].argmax()) == tok
            cur = torch.cat((cur, torch.tensor([[tok]])), dim=1)
    assert m.generate(ids, images, False, 1.0, 1.0, 3, out[0], wkv=oracle_wkv_state) == out[:1]       # the stop token ends it


def test_state_op_has_no_cpu_path():
    from visualrwkv_amd import wkv6
    r = torch.zeros(1, 16, 64, dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError):
        wkv6.RUN_CUDA_RWKV6_STATE(1, 16, 64, 1, r, r, r, r, torch.zeros(1, 64, dtype=torch.bfloat16), torch.zeros(1, 1, 64, 64))
