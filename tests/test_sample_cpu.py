"""Sampled generation on the CPU: VisualRWKV.generate / generate_stateful with do_sample=True (sampling.pick -> pick_torch off the GPU), on a
tiny model (C = 256, 3 layers, vocabulary 1000; the WKV kernels replaced by the oracle's recurrence as in tests/test_stateful_cpu.py), and
pick_torch itself against the fp64 oracle of tests/test_sample_shapes.py on that module's exact cases."""
import math
from types import SimpleNamespace

import pytest
import torch

from tests.test_sample_shapes import U_TOP, Ref, edges, spread
from tests.test_stateful_cpu import lm_args, oracle_kernels      # noqa: F401  (fixture)

N_NEW = 6


@pytest.fixture()
def model(oracle_kernels):      # noqa: F811
    from visualrwkv_amd.visual import VisualRWKV
    args = lm_args(n_embd=256, dim_att=256, vocab_size=1000, ctx_len=128, vision_towers=("dino",), vision_image_size=56,
                   vision_tower_kwargs={"dino": dict(depth=1, dim=64, heads=1)})
    torch.manual_seed(0)
    m = VisualRWKV(args).double().eval()
    with torch.no_grad():
        for b in m.rwkv.blocks:
            b.att.output.weight.normal_(0, 0.05)
            b.ffn.value.weight.normal_(0, 0.05)
        m.rwkv.head.weight.mul_(4.0)                         # peaked enough that a nucleus is not the whole vocabulary
    ids = torch.randint(0, 256, (1, 27))
    images = {"dino": torch.randn(1, 3, 56, 56, dtype=torch.float64)}
    return m, ids, images


def gen(seed):
    return torch.Generator().manual_seed(seed)


def test_sampled_generation_returns(model):
    m, ids, images = model
    for fn in (m.generate, m.generate_stateful):
        toks, lgs, prs = fn(ids, images, True, 1.0, 0.9, N_NEW, -7, generator=gen(1))
        assert len(toks) == len(lgs) == len(prs) == N_NEW
        assert all(isinstance(t, int) and 0 <= t < 1000 for t in toks) and all(0 < p <= 1 for p in prs)


def test_top_p_zero_is_greedy(model):
    m, ids, images = model
    for fn in (m.generate, m.generate_stateful):
        want = fn(ids, images, False, 1.0, 1.0, N_NEW, -7)
        got = fn(ids, images, True, 1.3, 0.0, N_NEW, -7, generator=gen(2))
        assert got[0] == want[0] and got[1] == want[1]
        assert got[2] == pytest.approx(want[2], rel=1e-12)


def test_the_generator_decides(model):
    m, ids, images = model
    for fn in (m.generate, m.generate_stateful):
        a = fn(ids, images, True, 2.0, 1.0, N_NEW, -7, generator=gen(3))
        b = fn(ids, images, True, 2.0, 1.0, N_NEW, -7, generator=gen(3))
        c = fn(ids, images, True, 2.0, 1.0, N_NEW, -7, generator=gen(4))
        assert a == b and a[0] != c[0]


def test_stop_token_ends_a_sampled_run(model):
    m, ids, images = model
    full = m.generate_stateful(ids, images, True, 1.0, 0.9, N_NEW, -7, generator=gen(5))
    cut = m.generate_stateful(ids, images, True, 1.0, 0.9, N_NEW, full[0][2], generator=gen(5))
    n = full[0].index(full[0][2]) + 1
    assert cut[0] == full[0][:n] and cut[1] == full[1][:n]


def _in_nucleus(logits_row, token, top_p):
    return bool(Ref(logits_row, 1.0, top_p).K[token])


def test_tokens_lie_in_the_nucleus_of_their_logits(model):
    """The logits recomputed by full passes over prompt + tokens so far: generate's re-padded pass; generate_stateful's fixed left pad."""
    m, ids, images = model
    top_p = 0.6
    samples = {"input_ids": ids, "images": images, "labels": ids}
    with torch.no_grad():
        x0, _ = m.preparing_embedding(samples)
        toks, lgs, _ = m.generate(ids, images, True, 1.5, top_p, N_NEW, -7, generator=gen(6))
        x, sizes = x0, []
        for t, lg in zip(toks, lgs):
            row = m.rwkv(x)[0, -1]
            assert _in_nucleus(row, t, top_p) and float(row[t]) == pytest.approx(lg, rel=1e-9)
            sizes.append(int(Ref(row, 1.0, top_p).K.sum()))
            x = torch.cat((x, m.rwkv.emb(torch.tensor([[t]]))), dim=1)
        assert max(sizes) < 1000 and max(sizes) > 1, sizes          # the nucleus is neither everything nor the argmax alone
        toks, lgs, _ = m.generate_stateful(ids, images, True, 1.5, top_p, N_NEW, -7, generator=gen(7))
        x = m.rwkv.pad_left(x0, 5)
        for t in toks[:-1]:
            x = torch.cat((x, m.rwkv.emb(torch.tensor([[t]]))), dim=1)
        rows = m.rwkv.forward_stateful(x, None)[0][0, 31:]
        for row, t, lg in zip(rows, toks, lgs):
            assert _in_nucleus(row, t, top_p) and float(row[t]) == pytest.approx(lg, rel=1e-9)


def test_several_rows(model):
    """B = 2 on the CPU path: every entry holds B values, and the rows take their own u."""
    m, ids, images = model
    ids2 = torch.cat((ids, ids))
    images2 = {"dino": torch.cat((images["dino"], images["dino"]))}
    g = gen(8)
    u = torch.rand(N_NEW, 2, generator=gen(8))
    toks, lgs, prs = m.generate_stateful(ids2, images2, True, 1.0, 0.9, N_NEW, -7, generator=g)
    assert len(toks) == N_NEW and all(len(t) == 2 for t in toks)
    assert any(a != b for a, b in toks) or bool((u[:, 0] == u[:, 1]).all())


def test_argument_errors(model):
    from visualrwkv_amd import sampling
    m, ids, images = model
    l = torch.zeros(1, 8)
    for tau, top_p in ((0.0, 0.9), (-1.0, 0.9), (1.0, -0.1), (math.nan, 0.5)):
        with pytest.raises(ValueError):
            sampling.pick(l, tau, top_p, torch.tensor([0.5]))
        with pytest.raises(ValueError):
            sampling.pick_torch(l, tau, top_p, torch.tensor([0.5]))
        for fn in (m.generate, m.generate_stateful):
            with pytest.raises(ValueError):
                fn(ids, images, True, tau, top_p, 2, -7)
    with pytest.raises(ValueError):
        sampling.pick(l, 1.0, 0.9, torch.tensor([0.5]), emb=torch.zeros(8, 8))


def test_prototype_counts_the_header_arguments():
    """hip_lib's table against the header: the entry's argument count, stream included (tests/test_capi.py compares the names)."""
    import os
    import re
    from visualrwkv_amd import hip_lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "visualrwkv_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    args = re.search(r"int\s+vrwkv_sample_pick_bf16\s*\(([^)]*)\)", hdr).group(1).split(",")
    res, argtypes = hip_lib.PROTOTYPES["vrwkv_sample_pick_bf16"]
    assert len(argtypes) == len(args) == 11 and "stream" in args[-1]


def test_v6_still_refuses():
    from visualrwkv_amd.visual6 import VisualRWKV6
    me = SimpleNamespace(args=SimpleNamespace(image_state=1))
    with pytest.raises(NotImplementedError):
        VisualRWKV6.generate(me, None, None, True, 1.0, 1.0, 2, -1)
    with pytest.raises(NotImplementedError):
        VisualRWKV6.generate_stateful(me, None, None, True, 1.0, 1.0, 2, -1)


# ------------------------------------------------------------------------------------------------ pick_torch on the exact cases
def _pick(row, tau, top_p, us):
    from visualrwkv_amd import sampling
    logits = row.view(1, -1).repeat(len(us), 1)
    emb = torch.randn(row.numel(), 8, generator=gen(9)).bfloat16()
    x_out = torch.zeros(len(us), 1, 8, dtype=torch.bfloat16)
    tk, lt, pt = sampling.pick_torch(logits, tau, top_p, torch.tensor(us, dtype=torch.float64), emb, x_out)
    ref = Ref(row, tau, top_p)
    assert tk.dtype == torch.int32 and torch.equal(tk.long(), ref.token(us)), (tk.tolist(), ref.token(us).tolist())
    assert torch.equal(lt, row.float()[tk.long()]) and torch.equal(x_out[:, 0], emb[tk.long()])
    assert torch.allclose(pt.double(), ref.p[tk.long()], rtol=1e-5, atol=0)
    return ref, tk.tolist()


@pytest.mark.parametrize("V", [8, 2056])
def test_pick_torch_on_the_exact_cases(V):
    base = torch.randn(V, generator=gen(7)).clamp_(-3, 3)
    for at in edges(V):                                      # needle
        row = base.clone()
        row[at] = 43.0
        for top_p in (0.0, 0.5, 1.0):
            _, tk = _pick(row.bfloat16(), 1.0, top_p, [0.0, 0.5, U_TOP])
            assert tk == ([at] * 3 if top_p < 1 or at == 0 else [0, at, at])
    for n in (2, 3) if V == 8 else (2, 3, 64, 65):           # flat nucleus
        pos = spread(V, n)
        row = torch.full((V,), -26.0)
        row[pos] = 4.0
        for tau in (0.5, 1.0, 2.0):
            _, tk = _pick(row.bfloat16(), tau, 0.9, [(j + 0.5) / n for j in range(n)] + [U_TOP])
            assert tk == pos + [pos[-1]]
    row = torch.full((V,), 1.5).bfloat16()                   # top_p >= 1 on a flat row: every index
    for top_p in (1.0, 1.5):
        _, tk = _pick(row, 0.7, top_p, [(i + 0.5) / V for i in range(V)])
        assert tk == list(range(V))
    row = base.clone()                                       # top_p = 0 with a tied maximum
    row[[2, V - 3]] = 6.0
    _, tk = _pick(row.bfloat16(), 1.0, 0.0, [0.0, 0.49, 0.51, U_TOP])
    assert tk == [2, 2, V - 3, V - 3]
    row = base.clone()                                       # -inf entries
    row[[0, 1, V - 1]] = -math.inf
    ref, tk = _pick(row.bfloat16(), 1.0, 1.0, [0.0, 0.3, 0.7, U_TOP])
    assert tk[0] == 2 and not {0, 1, V - 1} & set(tk)


def test_pick_torch_ties_and_temperature():
    V = 2056
    l1, l2 = spread(V, 13)[:2], spread(V, 13)[2:8]
    row = torch.full((V,), -5.0)
    row[l1], row[l2] = 10.0, 9.0
    us = [(i + 0.5) / 64 for i in range(64)]
    ref, tk = _pick(row.bfloat16(), 1.0, 0.6, us)
    assert ref.clear_of_cdf(us) and set(l2) <= set(tk) <= set(l1 + l2)
    for tau in (0.5, 2.0):
        row = torch.full((V,), -28.0)
        row[l1], row[l2] = 2.0, 1.0
        ref, tk = _pick(row.bfloat16(), tau, 0.99, us)
        assert ref.clear_of_cdf(us)
        share = sum(t in l1 for t in tk) / 64
        assert abs(share - 2 / (2 + 6 * math.exp(-1.0 / tau))) <= 8 / 64
