"""Training a long row in segments (VisualRWKV.train_step_cut, rwkv7.TrainCarry) on an fp64 unfused model on CPU tensors: what crosses a cut
-- the ln1 / ln2 output of the last token and the WKV state, per layer -- carries gradients, so the cut step IS the uncut step.  Bounds: 1e-9
relative, fp64 round-off under another summation order (per-segment partial sums of the loss and of every parameter gradient)."""
from types import SimpleNamespace

import pytest
import torch

from oracle.wkv7_oracle import wkv7_naive

B, T, V = 2, 64, 300


@pytest.fixture(autouse=True)
def _fp64_stateless_op(monkeypatch):
    """The stateless op (what the UNCUT model runs) has no fp64 form: the oracle's recurrence stands in for it, under autograd.  The cut
    side runs RUN_CUDA_RWKV7g_state, whose CPU form is this package's own fp64 recurrence."""
    from visualrwkv_amd import rwkv7

    def naive(q, w, k, v, a, b):                 # RUN_CUDA_RWKV7g's argument order
        Bq, Tq, HC = q.shape
        return wkv7_naive(*[i.view(Bq, Tq, HC // 64, 64) for i in (w, q, k, v, a, b)])[0].reshape(Bq, Tq, HC)
    monkeypatch.setattr(rwkv7, "RUN_CUDA_RWKV7g", naive)


def _visual(n_layer=3, **kw):
    from visualrwkv_amd.visual import VisualRWKV
    d = dict(n_embd=128, n_layer=n_layer, dim_att=128, head_size_a=64, head_size_divisor=8, vocab_size=V, dropout=0, grad_cp=0, ctx_len=T,
             num_token_per_image=16, vision_towers=("dino",), vision_image_size=56, load_model="", proj_type="mlp", weight_decay=0.0, fused=False,
             vision_tower_kwargs={"dino": dict(depth=1, dim=64, heads=1)})
    d.update(kw)
    torch.manual_seed(0)
    m = VisualRWKV(SimpleNamespace(**d))
    with torch.no_grad():                        # zero-initialised projections would hide what crosses a cut
        for b in m.rwkv.blocks:
            b.att.output.weight.normal_(0, 0.05)
            b.ffn.value.weight.normal_(0, 0.05)
            if hasattr(b.att, "time_state"):
                b.att.time_state.normal_(0, 0.3)
    return m.double()


def _batch(t=T):
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, V, (B, t), generator=g)
    labels = ids.clone()
    labels[0, :5] = -100                         # unequal label counts per segment and per sample
    labels[1, :19] = -100
    labels[0, 27:30] = -100
    labels[:, 33:49] = -100                      # rows 32 .. 47 predict tokens 33 .. 48: the third 16-token segment has no label at all
    labels[1, 60:] = -100
    return {"input_ids": ids, "labels": labels}


def _close(a, b, tol=1e-9):
    return float((a - b).norm()) <= tol * float(b.norm())


def _uncut(m, batch):
    m.zero_grad(set_to_none=True)
    loss = m.training_step(batch)
    loss.backward()
    return loss.detach(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}


def _cut(m, batch, seg_len, **kw):
    m.zero_grad(set_to_none=True)
    loss = m.train_step_cut(batch, seg_len, **kw)
    assert not loss.requires_grad
    return loss, {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}


def _same(got, ref, tol=1e-9):
    assert abs(float(got[0]) - float(ref[0])) <= tol * abs(float(ref[0])), (float(got[0]), float(ref[0]))
    assert set(got[1]) == set(ref[1]) and len(ref[1]) > 40
    for n, g in ref[1].items():
        assert _close(got[1][n], g, tol), (n, float((got[1][n] - g).norm()), float(g.norm()))


def test_chained_carry_forward_equals_the_uncut_logits():
    from visualrwkv_amd.rwkv7 import TrainCarry
    m = _visual()
    x = m.rwkv.emb(_batch()["input_ids"])
    with torch.no_grad():
        whole = m.rwkv(x)
        carry, parts = TrainCarry(3), []
        for a in (0, 16, 48):                                    # segments of 16, 32 and 16 tokens
            b = {0: 16, 16: 48, 48: 64}[a]
            logits, carry = m.rwkv(x[:, a:b], carry=carry)
            parts.append(logits)
        assert all(t is not None for layer in carry.layers for t in layer) and len(carry.tensors()) == 9
        assert _close(torch.cat(parts, dim=1), whole)
        # without a carry the second segment is another function (it sees nothing of the first)
        assert not _close(m.rwkv(x[:, 16:48]), whole[:, 16:48], 1e-3)


@pytest.mark.parametrize("grad_cp", [0, 1])
@pytest.mark.parametrize("seg_len", [32, 16, 64, 48])
def test_cut_step_is_the_uncut_step(seg_len, grad_cp):
    """K = 2, 4, 1, and two unequal segments (48 + 16): the loss and every parameter gradient of training_step + backward."""
    m = _visual(grad_cp=grad_cp)
    batch = _batch()
    ref = _uncut(m, batch)
    _same(_cut(m, batch, seg_len), ref)


@pytest.mark.parametrize("seg_len", [32, 16])
def test_cut_step_with_state_tuning(seg_len):
    """args.state_tune: segment 0 starts from time_state, whose gradient arrives through every cut."""
    m = _visual(n_layer=2, state_tune=1)
    batch = _batch()
    ref = _uncut(m, batch)
    got = _cut(m, batch, seg_len)
    assert "rwkv.blocks.0.att.time_state" in ref[1] and float(ref[1]["rwkv.blocks.1.att.time_state"].norm()) > 0
    _same(got, ref)
    m.freeze_for_state_tuning()                                  # only the states train: no gradient reaches the embedding
    ref = _uncut(m, batch)
    got = _cut(m, batch, seg_len)
    assert set(ref[1]) == {f"rwkv.blocks.{i}.att.time_state" for i in range(2)} == set(got[1])
    for n, g in ref[1].items():
        assert _close(got[1][n], g), n


def test_truncated_mode():
    """truncate=True is truncated back-propagation through time: a hand-written loop over the segments with detached carries.  With one
    segment nothing is truncated: it equals the exact mode and the uncut step."""
    from visualrwkv_amd.rwkv7 import TrainCarry
    m = _visual(n_layer=2)
    batch = _batch()
    got = _cut(m, batch, 16, truncate=True)
    m.zero_grad(set_to_none=True)
    x = m.rwkv.emb(batch["input_ids"])
    carry, total = TrainCarry(2), 0.0
    for a in range(0, T, 16):
        logits, nxt = m.rwkv(x[:, a:a + 16], carry=carry)
        loss = m.loss_from_logits(logits, batch["labels"], None, (a, a + 16))
        loss.backward(retain_graph=True)                         # the embedding's graph is shared by the segments
        total += float(loss.detach())
        carry = nxt.detach()
    hand = (torch.tensor(total, dtype=torch.float64), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})
    _same(got, hand)
    exact = _cut(m, batch, 16)
    assert not _close(got[1]["rwkv.blocks.0.att.key.weight"], exact[1]["rwkv.blocks.0.att.key.weight"], 1e-4)      # truncation drops something
    assert abs(float(got[0]) - float(exact[0])) <= 1e-9 * abs(float(exact[0]))                                    # ... but not from the loss
    ref = _uncut(m, batch)
    _same(_cut(m, batch, 64, truncate=True), ref)
    _same(_cut(m, batch, 64), ref)


def test_window_loss_shares_add_up():
    """loss_from_logits with a window: whole-row weights and L2Wrap factor, so the shares of any cut add up to the row's loss and the logits'
    gradient is the uncut one."""
    from visualrwkv_amd.visual import VisualRWKV
    g = torch.Generator().manual_seed(2)
    logits = torch.randn(B, T, V, generator=g, dtype=torch.float64).requires_grad_(True)
    labels = _batch()["labels"]
    whole = VisualRWKV.loss_from_logits(logits, labels)
    whole.backward()
    gref, logits.grad = logits.grad.clone(), None
    parts = [VisualRWKV.loss_from_logits(logits[:, a:b], labels, None, (a, b)) for a, b in ((0, 16), (16, 48), (48, 64))]
    sum(parts).backward()
    assert abs(float(sum(parts).detach()) - float(whole.detach())) <= 1e-12 * abs(float(whole.detach()))
    assert _close(logits.grad, gref, 1e-12)


def test_what_is_refused():
    from visualrwkv_amd.rwkv7 import TrainCarry
    from visualrwkv_amd.wkv7 import PackedLayout
    m = _visual(n_layer=2)
    with pytest.raises(ValueError):
        m.train_step_cut(_batch(40), 16)                         # T not a multiple of 16
    with pytest.raises(ValueError):
        m.train_step_cut(_batch(), 24)                           # seg_len not a multiple of 16
    with pytest.raises(ValueError):
        m.train_step_cut(_batch(), 0)
    packed = dict(_batch(), seg_lens=[[32, 32], [48, 16]], n_samples=4)
    with pytest.raises(NotImplementedError):
        m.train_step_cut(packed, 32)
    x = m.rwkv.emb(_batch()["input_ids"])
    with pytest.raises(NotImplementedError):
        m.rwkv(x, layout=PackedLayout([[32, 32], [48, 16]], T), carry=TrainCarry(2))
    with pytest.raises(ValueError):
        m.rwkv(x[:, :24], carry=TrainCarry(2))                   # a segment is whole chunks
    with pytest.raises(ValueError):
        m.rwkv(x, carry=TrainCarry(3))                           # another model's carry
    # a call without a carry returns what it returned before: logits alone, (hidden, pad) with hidden_only
    assert torch.is_tensor(m.rwkv(x)) and len(m.rwkv(x, hidden_only=True)) == 2
