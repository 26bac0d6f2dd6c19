"""Packed rows at the model level on CPU tensors: the eager Blocks with a wkv7.PackedLayout (masked token shift, the WKV7 op once per
segment) against the same samples run as rows of their own, and the per-segment loss."""
from types import SimpleNamespace

import pytest
import torch

from oracle.wkv7_oracle import rel_rms

LENS = [32, 16, 48]


def _lm(**kw):
    from visualrwkv_amd.rwkv7 import RWKV
    d = dict(n_embd=128, n_layer=2, dim_att=128, head_size_a=64, head_size_divisor=8, vocab_size=300, dropout=0,
             grad_cp=0, ctx_len=96, load_model="", num_token_per_image=16, proj_type="mlp")
    d.update(kw)
    torch.manual_seed(3)
    m = RWKV(SimpleNamespace(**d))
    with torch.no_grad():                        # zero-initialised projections would hide what crosses a boundary
        for b in m.blocks:
            b.att.output.weight.normal_(0, 0.05)
            b.ffn.value.weight.normal_(0, 0.05)
    return m.float()


def _batch():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, sum(LENS), 128, generator=g)
    labels = torch.randint(0, 300, (1, sum(LENS)), generator=g)
    t = 0
    for n in LENS:
        labels[0, t] = -100                      # what pack_batches does: nothing in a segment predicts its first token
        labels[0, t + n - 3:t + n] = -100        # and some padding at its end
        t += n
    return x, labels


def _grads(m):
    return {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("grad_cp", [0, 1])
def test_packed_row_equals_the_samples_run_as_rows_of_their_own(grad_cp):
    """Loss and every parameter gradient.  Both sides apply the SAME packed loss to (1, 96, V) logits -- the separate runs' logits are
    concatenated first -- so L2Wrap's 1 / (B T) is the same.  Bound: 1e-5 rel-RMS, what tests/test_state_tuning_cpu.py:73 holds two fp32
    evaluations of the same math through different paths to."""
    from visualrwkv_amd.visual import VisualRWKV
    from visualrwkv_amd.wkv7 import PackedLayout
    x, labels = _batch()
    lay = PackedLayout([LENS], sum(LENS))
    m = _lm(grad_cp=grad_cp)
    logits_p = m(x, layout=lay)
    loss_p = VisualRWKV.loss_from_logits(logits_p, labels, lay)
    loss_p.backward()
    gp = _grads(m)
    m.zero_grad(set_to_none=True)
    parts, t = [], 0
    for n in LENS:
        parts.append(m(x[:, t:t + n].contiguous()))
        t += n
    logits_s = torch.cat(parts, dim=1)
    loss_s = VisualRWKV.loss_from_logits(logits_s, labels, lay)
    loss_s.backward()
    gs = _grads(m)
    assert rel_rms(logits_p.detach(), logits_s.detach()) < 1e-5
    lp, ls = float(loss_p.detach()), float(loss_s.detach())
    assert abs(lp - ls) < 1e-5 * abs(ls), (lp, ls)
    assert set(gp) == set(gs) and len(gp) > 40
    for n in gs:
        assert rel_rms(gp[n], gs[n]) < 1e-5, (n, rel_rms(gp[n], gs[n]))


def test_packing_matters():
    """The same row WITHOUT a layout: segment 0 is untouched (nothing precedes it), segments 1 and 2 see what came before."""
    from visualrwkv_amd.wkv7 import PackedLayout
    x, _ = _batch()
    m = _lm()
    with torch.no_grad():
        packed = m(x, layout=PackedLayout([LENS], sum(LENS)))
        plain = m(x)
    a, b = LENS[0], LENS[0] + LENS[1]
    assert rel_rms(plain[:, :a], packed[:, :a]) < 1e-5
    assert rel_rms(plain[:, a:b], packed[:, a:b]) > 1e-2
    assert rel_rms(plain[:, b:], packed[:, b:]) > 1e-2


def test_packed_loss_is_the_reference_loss_per_segment():
    """One segment per row and n_samples = B: the packed loss is the reference's loss on that batch, to round-off."""
    from visualrwkv_amd.visual import VisualRWKV
    from visualrwkv_amd.wkv7 import PackedLayout
    g = torch.Generator().manual_seed(1)
    logits = torch.randn(3, 32, 50, generator=g)
    labels = torch.randint(0, 50, (3, 32), generator=g)
    labels[:, 0] = -100
    labels[1, 20:] = -100
    labels[2, :] = -100                                          # a row without a valid label counts as a sample of loss 0
    ref = VisualRWKV.loss_from_logits(logits, labels)
    got = VisualRWKV.loss_from_logits(logits, labels, PackedLayout([[32]] * 3, 32))
    assert torch.allclose(got, ref, rtol=1e-6, atol=1e-7)
    # a pad-only tail segment is not a sample: n_samples divides, the segment adds nothing
    lay = PackedLayout([[16, 16]], 32, n_samples=1)
    lab = labels[:1].clone(); lab[0, 16:] = -100
    one = VisualRWKV.loss_from_logits(logits[:1], lab, lay)
    ref1 = VisualRWKV.loss_from_logits(logits[:1, :16], lab[:, :16])
    assert torch.allclose(one, ref1, rtol=1e-6, atol=1e-7)


def test_state_tune_with_a_layout_is_refused():
    from visualrwkv_amd.wkv7 import PackedLayout
    x, _ = _batch()
    with pytest.raises(NotImplementedError):
        _lm(state_tune=1)(x, layout=PackedLayout([LENS], sum(LENS)))


def test_forward_reads_seg_lens():
    from visualrwkv_amd.visual import VisualRWKV
    x, labels = _batch()
    holder = SimpleNamespace(args=SimpleNamespace(fused=False), rwkv=_lm())
    holder.preparing_embedding = lambda samples: (x, samples["labels"])
    holder.packed_layout = VisualRWKV.packed_layout
    holder.loss_from_logits = VisualRWKV.loss_from_logits
    batch = {"input_ids": torch.zeros(1, sum(LENS), dtype=torch.long), "labels": labels, "seg_lens": [LENS], "n_samples": 3}
    logits, targets = VisualRWKV.forward(holder, batch)
    from visualrwkv_amd.wkv7 import PackedLayout
    want = VisualRWKV.loss_from_logits(holder.rwkv(x, layout=PackedLayout([LENS], sum(LENS))), labels, PackedLayout([LENS], sum(LENS)))
    got = VisualRWKV.loss_from_logits(logits, targets, VisualRWKV.packed_layout(batch, x.device))
    assert torch.equal(got, want)
