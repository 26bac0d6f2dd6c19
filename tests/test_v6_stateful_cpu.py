"""Stateful RWKV-6 inference on CPU in fp32: RWKV6State, RWKV.forward_stateful (module path) and VisualRWKV6.generate_stateful for both
models (args.image_state = 1: the image as every layer's initial WKV state; 0: the bidirectional model with the image span in the
context), around the oracle-backed stand-in for RUN_CUDA_RWKV6_STATE.  The models are the two-layer ones of tests/test_v6_state_cpu.py
(layer 1 is an odd layer: it reads the image span right to left), their weights taken to fp32.

A stateful pass is the same arithmetic as the one pass, cut at other places: fp32 throughout, the oracle recurrence in fp64 from an fp32
state, so the two differ by fp32 roundings of the handed-over state and of matrix products of other shapes -- 1e-5 rel-RMS on the logits."""
import pytest
import torch

from oracle.wkv7_oracle import rel_rms
from tests.test_v6_cpu import _oracle_wkv
from tests.test_v6_state_cpu import _samples, _visual, gold, oracle_wkv_state  # noqa: F401  (gold: the module's fixture)

TOL = 1e-5


def _model(gold, image_state):
    return _visual(gold, image_state=image_state).float().eval()


def _one(gold):
    s = _samples(gold)
    return s["input_ids"][:1], s["images"][:1].float()


@pytest.mark.parametrize("image_state", [1, 0])
def test_forward_stateful_splits_equal_one_pass(gold, image_state):
    """The text stack alone, B = 3, T = 24: any split of the rows gives the one pass's logits and the same final state."""
    rwkv = _model(gold, image_state).rwkv
    g = torch.Generator().manual_seed(11 + image_state)
    B, T, C = 3, 24, rwkv.args.n_embd
    x = torch.randn(B, T, C, generator=g)
    with torch.no_grad():
        want = rwkv(x, _oracle_wkv())
    full, st_full = rwkv.forward_stateful(x, None, wkv=oracle_wkv_state)
    assert rel_rms(full, want) < TOL
    assert st_full.n_tokens == T
    for split in ([T], [5, 1, 1, T - 7], [1, T - 1]):
        state, outs, t0 = None, [], 0
        for n in split:
            lg, state = rwkv.forward_stateful(x[:, t0:t0 + n], state, wkv=oracle_wkv_state)
            assert lg.shape == (B, n, rwkv.args.vocab_size)
            outs.append(lg)
            t0 += n
        assert rel_rms(torch.cat(outs, dim=1), want) < TOL, split
        assert state.n_tokens == T
        for a, b in zip(state.S + state.att_x + state.ffn_x, st_full.S + st_full.att_x + st_full.ffn_x):
            assert rel_rms(a, b) < TOL, split
    last, _ = rwkv.forward_stateful(x, None, last_only=True, wkv=oracle_wkv_state)
    assert last.shape == (B, rwkv.args.vocab_size) and rel_rms(last, want[:, -1]) < TOL


def test_state_layout_and_carried_rows(gold):
    """S is RUN_CUDA_RWKV6_STATE's (B,H,64,64) fp32 [key][value]; the carried rows are the last ln1 / ln2 rows."""
    rwkv = _model(gold, 1).rwkv
    x = torch.randn(2, 6, rwkv.args.n_embd, generator=torch.Generator().manual_seed(3))
    _, st = rwkv.forward_stateful(x, None, wkv=oracle_wkv_state)
    H = rwkv.args.dim_att // 64
    assert all(S.shape == (2, H, 64, 64) and S.dtype == torch.float32 for S in st.S)
    blk = rwkv.blocks[0]
    with torch.no_grad():
        h = blk.ln1(blk.ln0(x))
        _, s_ref = blk.att.forward_state(h, None, oracle_wkv_state)
    assert torch.equal(st.att_x[0], h[:, -1])
    assert rel_rms(st.S[0], s_ref) < TOL


def test_generate_stateful_returns_generates_tokens(gold):
    """image_state = 1: the tokens `generate` gives; the stop token ends it; sampling is not built."""
    m = _model(gold, 1)
    ids, images = _one(gold)
    want = m.generate(ids, images, False, 1.0, 1.0, 5, -1, wkv=oracle_wkv_state)
    got = m.generate_stateful(ids, images, False, 1.0, 1.0, 5, -1, wkv=oracle_wkv_state)
    assert len(want) == 5 and got == want
    assert m.generate_stateful(ids, images, False, 1.0, 1.0, 5, want[1], wkv=oracle_wkv_state) == want[:want.index(want[1]) + 1]
    with pytest.raises(NotImplementedError):
        m.generate_stateful(ids, images, True, 1.0, 1.0, 2, -1, wkv=oracle_wkv_state)


def test_generate_stateful_bidirectional_is_the_argmax_of_the_last_row(gold):
    """image_state = 0, which `generate` refuses: each token is the argmax of bidirectional_forward's last row on the prompt extended so
    far (the check of test_v6_state_cpu.py::test_generate_is_the_argmax_of_the_last_row), and the logits agree to TOL."""
    m = _model(gold, 0)
    ids, images = _one(gold)
    with pytest.raises(NotImplementedError):
        m.generate(ids, images, False, 1.0, 1.0, 2, -1)                       # unchanged: the stateless method stays unbuilt for this model
    out = m.generate_stateful(ids, images, False, 1.0, 1.0, 4, -1, wkv=oracle_wkv_state)
    assert len(out) == 4
    with torch.no_grad():
        cur = ids
        for tok in out:
            x, _, _ = m.preparing_embedding({"input_ids": cur, "images": images, "labels": torch.full_like(cur, -100)}, truncate=False)
            assert m.img_end - m.img_start == 4 and m.img_end < x.shape[1]      # a span of 4 rows inside the context, text behind it
            row = m.bidirectional_forward(x, _oracle_wkv())[0, -1]
            assert int(row.argmax()) == tok
            cur = torch.cat((cur, torch.tensor([[tok]])), dim=1)
        # the prefill's own logits against the one pass
        x, _, _ = m.preparing_embedding({"input_ids": ids, "images": images, "labels": torch.full_like(ids, -100)}, truncate=False)
        want = m.bidirectional_forward(x, _oracle_wkv())[:, -1]
        got, state = m.prefill_state(ids, images, oracle_wkv_state)
    assert rel_rms(got, want) < TOL and state.n_tokens == x.shape[1]
    with pytest.raises(NotImplementedError):
        m.generate_stateful(ids, images, True, 1.0, 1.0, 2, -1, wkv=oracle_wkv_state)
