"""Penalised sampled generation on the MI355X: presence / count penalties and the token ban inside the pick kernel at the end of the
captured decode step (GraphDecoder(sampled=True, penalised=True)) against the same call without the graph, against the argmax of the
penalised logits of an unsampled decoder run, and call after call.  The tiny model of tests/test_sample_gpu.py, bf16, fused."""
import pytest
import torch

from tests.test_sample_gpu import _quiet, gen, model      # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

N_NEW = 16
PEN = dict(presence_penalty=0.4, count_penalty=0.4, penalty_decay=0.996)


def _prompt(seed, B):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, 256, (B, 27), generator=g).cuda()
    return ids, {"dino": torch.randn(B, 3, 56, 56, generator=g).cuda().bfloat16()}


def _rows(toks, B):
    """The returned token list as one list per batch row."""
    return [list(toks)] if B == 1 else [[t[b] for t in toks] for b in range(B)]


def _prefill(model, ids, images):
    from visualrwkv_amd.rwkv7 import CHUNK_LEN
    samples = {"input_ids": ids, "images": images, "labels": ids}
    x, _ = model.preparing_embedding(samples)
    rem = x.size(1) % CHUNK_LEN
    return model.rwkv.forward_stateful(model.rwkv.pad_left(x, CHUNK_LEN - rem if rem else 0), None, last_only=True)


@pytest.mark.parametrize("B", [1, 3])
def test_graph_equals_the_eager_path(model, B):
    ids, images = _prompt(40 + B, B)
    first = _rows(model.generate_stateful(ids, images, False, 1.0, 1.0, 1, -7)[0], 1)[0] if B == 1 else []
    for tau, top_p, ban in ((1.0, 0.9, ()), (1.4, 1.0, tuple(first) + (5, 17))):
        a = model.generate_stateful(ids, images, True, tau, top_p, N_NEW, -7, use_graph=True, generator=gen(B), token_ban=ban, **PEN)
        b = model.generate_stateful(ids, images, True, tau, top_p, N_NEW, -7, use_graph=False, generator=gen(B), token_ban=ban, **PEN)
        assert len(a[0]) == N_NEW and a == b
        assert not set(ban) & {t for row in _rows(a[0], B) for t in row}


def _assert_penalised_argmax(model, ids, images, rows, presence):
    """Every token of `rows` (one list per batch row) has the largest penalised logit of its step, on an unsampled captured decoder fed with
    those tokens: the penalty on the logits in torch (fp32, rounded to bf16) at every token seen so far.  (Where two penalised logits tie for
    the maximum, top_p = 0 keeps both and u decides: either is right.)"""
    rwkv = model.rwkv
    with torch.no_grad():
        logits, state = _prefill(model, ids, images)
        dec = rwkv.decoder_for(state)
        B = logits.size(0)
        seen = torch.zeros(B, logits.size(1), device="cuda")
        for i in range(len(rows[0])):
            out = torch.where(seen > 0, (logits.float() - presence).bfloat16(), logits).float()
            tk = torch.tensor([r[i] for r in rows], device="cuda")
            assert torch.equal(out[torch.arange(B), tk], out.max(dim=-1).values), f"step {i}: {tk.tolist()} is not the penalised argmax"
            seen[torch.arange(B), tk] = 1.0
            logits = dec(rwkv.emb(tk.view(B, 1))).clone()


@pytest.mark.parametrize("B", [1, 3])
def test_a_presence_penalty_ends_the_repeats(model, B):
    """top_p = 0 under a presence penalty of 128 (above every gap between two logits): no row produces a token twice, and every token is the
    argmax of the penalised logits of an unsampled decoder run.  The prompt is the first of 16 seeds on which the same call without
    penalties repeats a token -- asserted."""
    n = 48
    for seed in range(16):
        ids, images = _prompt(100 + seed, B)
        plain = model.generate_stateful(ids, images, True, 1.0, 0.0, n, -7, generator=gen(1))
        if any(len(set(r)) < n for r in _rows(plain[0], B)):
            break
    else:
        raise AssertionError("no candidate prompt repeats a token without penalties")
    runs = []
    for use_graph in (True, False):
        got = model.generate_stateful(ids, images, True, 1.0, 0.0, n, -7, use_graph=use_graph, generator=gen(1), presence_penalty=128.0,
                                      count_penalty=0.0, penalty_decay=1.0)
        assert all(len(r) == n and len(set(r)) == n for r in _rows(got[0], B)), use_graph
        runs.append(got)
    assert runs[0] == runs[1]
    _assert_penalised_argmax(model, ids, images, _rows(runs[0][0], B), 128.0)


@pytest.mark.parametrize("B", [1, 3])
def test_a_banned_first_token_never_appears(model, B):
    ids, images = _prompt(60 + B, B)
    logits, _ = _prefill(model, ids, images)
    first = logits.argmax(dim=-1).tolist()
    free = model.generate_stateful(ids, images, True, 1.0, 0.0, N_NEW, -7, generator=gen(2))
    took = torch.tensor([r[0] for r in _rows(free[0], B)], device="cuda")
    assert torch.equal(logits[torch.arange(B), took], logits.max(dim=-1).values)      # unbanned, the first token is a largest logit
    for use_graph in (True, False):
        got = model.generate_stateful(ids, images, True, 1.0, 0.0, N_NEW, -7, use_graph=use_graph, generator=gen(2), token_ban=first)
        assert not set(first) & {t for r in _rows(got[0], B) for t in r}, use_graph


def test_one_more_launch_per_step_and_it_is_the_penalised_entry(model, monkeypatch):
    from visualrwkv_amd import hip_lib
    from visualrwkv_amd.rwkv7 import GraphDecoder
    rwkv = model.rwkv
    x = torch.randn(1, 32, 256, generator=gen(4)).cuda().bfloat16()
    _, state = rwkv.forward_stateful(x, None, last_only=True)
    lib, calls = hip_lib.load(), []

    class Spy:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if not name.startswith("vrwkv_") or name == "vrwkv_strerror":
                return fn

            def wrapped(*a):
                calls.append(name)
                return fn(*a)
            return wrapped
    monkeypatch.setattr(hip_lib, "load", lambda: Spy())
    rwkv.forward_stateful(x[:, :1], state, last_only=True)
    greedy = list(calls)
    assert greedy and not [c for c in greedy if "sample_pick" in c]
    calls.clear()
    dec = GraphDecoder(rwkv, state, sampled=True, penalised=True)
    assert calls == (greedy + ["vrwkv_sample_pick_pen_bf16"]) * 3      # two warm-up steps and the capture
    assert dec.pick.occ.shape == (1, 1000) and not bool(dec.pick.occ.any()), "the capture's own picks are still counted"
    with pytest.raises(ValueError):
        GraphDecoder(rwkv, state, sampled=False, penalised=True)


def test_the_cache_keeps_both_sampled_decoders(model):
    rwkv = model.rwkv
    x = torch.randn(1, 32, 256, generator=gen(5)).cuda().bfloat16()
    _, state = rwkv.forward_stateful(x, None, last_only=True)
    plain, pen = rwkv.decoder_for(state, sampled=True), rwkv.decoder_for(state, sampled=True, penalised=True)
    assert plain is not pen and pen.penalised and not plain.penalised and plain.pick.occ is None
    assert rwkv.decoder_for(state, sampled=True) is plain and rwkv.decoder_for(state, sampled=True, penalised=True) is pen


@pytest.mark.parametrize("B", [1, 3])
def test_two_calls_in_a_row_are_equal(model, B):
    """The decoder's occ is reset at the start of a call: the second call does not see the first one's counts, nor another call's ban."""
    ids, images = _prompt(80 + B, B)
    a = model.generate_stateful(ids, images, True, 1.1, 0.9, N_NEW, -7, use_graph=True, generator=gen(6), **PEN)
    model.generate_stateful(ids, images, True, 1.1, 0.9, 4, -7, use_graph=True, generator=gen(7), token_ban=_rows(a[0], B)[0][:2], **PEN)
    b = model.generate_stateful(ids, images, True, 1.1, 0.9, N_NEW, -7, use_graph=True, generator=gen(6), **PEN)
    assert a == b
