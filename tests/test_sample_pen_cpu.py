"""Presence / count penalties, the token ban and stop lists on the CPU: sampling.pick_torch(occ=) against the contract of
vrwkv_sample_pick_pen_bf16 on the exact cases of tests/test_sample_pen_shapes.py (its host-made l' and occ: independent of sampling.py), and
VisualRWKV.generate / generate_stateful with the new arguments on the tiny CPU model of tests/test_sample_cpu.py against a loop of
forward_stateful, the applications' dict code (VisualRWKV-v7/v7.10/app/app_gpu.py:56-86) and pick_torch."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests.test_sample_cpu import N_NEW, gen, model      # noqa: F401  (model: fixture)
from tests.test_sample_pen_shapes import DYADIC, app_loop, lprime_host, occ_after_host, random_case, sparse_case
from tests.test_sample_shapes import U_TOP, edges
from tests.test_stateful_cpu import oracle_kernels      # noqa: F401  (fixture of `model`)


# ------------------------------------------------------------------------------------------------ pick_torch(occ=)
def pick_pen(logits, occ, tau, top_p, us, ap, ac, decay):
    """pick_torch under occ against pick_torch on the host-made l' and the contract's occ; returns the tokens and occ after the call."""
    from visualrwkv_amd import sampling
    u = torch.tensor(us, dtype=torch.float64)
    got_occ = occ.clone()
    tk, lt, pt = sampling.pick_torch(logits, tau, top_p, u, occ=got_occ, presence=ap, count=ac, decay=decay)
    tk2, lt2, pt2 = sampling.pick_torch(lprime_host(logits, occ, ap, ac), tau, top_p, u)
    assert torch.equal(tk, tk2) and torch.equal(lt, lt2) and torch.equal(pt, pt2)
    assert torch.equal(got_occ.view(torch.int32), occ_after_host(occ, tk.long(), decay).view(torch.int32))
    return tk.tolist(), lt.tolist(), got_occ


@pytest.mark.parametrize("V", [8, 2056])
def test_pick_torch_on_the_exact_cases(V):
    logits, occ = sparse_case(V, 3)                          # zero and sparse dyadic counts, a banned token per row
    for top_p in (0.0, 0.5, 1.0):
        for tau in (0.7, 1.0):
            tk, _, after = pick_pen(logits, torch.zeros(3, V), tau, top_p, [0.0, 0.5, U_TOP], **DYADIC)
            assert after.sum() == 3 and all(float(after[b, t]) == 1.0 for b, t in enumerate(tk))
            pick_pen(logits, occ, tau, top_p, [0.0, 0.5, U_TOP], **DYADIC)
    i, j = (3, 5) if V == 8 else (511, 512)                  # the penalty changes the winner, or ties it with the runner-up
    row = torch.randn(V, generator=gen(13)).clamp_(-3, 3)
    row[i], row[j] = 8.0, 7.0
    occ = torch.zeros(4, V)
    occ[1, i], occ[2, i], occ[3, i] = 4.0, 2.0, 2.0
    tk, lt, _ = pick_pen(row.bfloat16().view(1, V).repeat(4, 1), occ, 1.0, 0.0, [0.5, 0.5, 0.25, 0.75], **DYADIC)
    assert tk == [i, j, i, j] and lt == [8.0, 7.0, 7.0, 7.0]
    at = edges(V)[-2]                                        # bf16 rounding of l', ties to even
    for pen, want in ((2.0 ** -9, 1.0), (3 * 2.0 ** -9, 0.9921875), (2.0 ** -8, 0.99609375)):
        row = torch.full((V,), -6.0)
        row[at] = 1.0
        occ = torch.zeros(1, V)
        occ[0, at] = 1.0
        tk, lt, _ = pick_pen(row.bfloat16().view(1, V), occ, 1.0, 0.0, [0.5], pen, 0.0, 0.5)
        assert tk == [at] and lt == [want]
    row = torch.full((V,), 2.0)                              # -inf under a count; a banned maximum, through three calls
    row[0] = -math.inf
    row[V - 3], row[2] = 9.0, 8.0
    occ = torch.zeros(1, V)
    occ[0, 0], occ[0, V - 3] = 3.0, -1.0
    for call in range(3):
        tk, _, occ = pick_pen(row.bfloat16().view(1, V), occ, 1.0, 0.0, [0.5], 0.25, 0.125, 0.5)
        assert tk == [2] and float(occ[0, V - 3]) == -1.0
    tk, _, _ = pick_pen(row.bfloat16().view(1, V), occ, 1.0, 1.0, [0.0], **DYADIC)
    assert tk == [1]


def test_pick_torch_carries_the_counts_like_the_applications():
    V = 2056
    logits = (6 * torch.randn(1, V, generator=gen(21))).bfloat16().clamp_(-4, 4)
    for k, p in enumerate((7, 8, 1000)):
        logits[0, p] = 9.0 - 0.5 * k
    want = app_loop(logits[0], 6, 0.25, 1.5, 0.996)
    assert len({t for t, _ in want}) == 3
    occ = torch.zeros(1, V)
    for token, d in want:
        tk, _, occ = pick_pen(logits, occ, 1.0, 0.0, [0.5], 0.25, 1.5, 0.996)
        ref = torch.zeros(V)
        for t, c in d.items():
            ref[t] = float(c)
        assert tk == [token] and torch.equal(occ[0].view(torch.int32), ref.view(torch.int32))


def test_pick_torch_random_rows():
    logits, occ, _ = random_case(2056, 3)
    pick_pen(logits, occ, 0.9, 0.9, [0.1, 0.5, 0.9], 0.3, 0.1, 0.996)


def test_pick_takes_occ_off_the_gpu():
    """sampling.pick on CPU rows is pick_torch, occ included; occ of another shape or dtype is refused."""
    from visualrwkv_amd import sampling
    logits, occ = sparse_case(2056, 3)
    a, b = occ.clone(), occ.clone()
    u = torch.tensor([0.2, 0.5, 0.8])
    got = sampling.pick(logits, 0.8, 0.9, u, occ=a, presence=0.5, count=0.25, decay=0.5)
    want = sampling.pick_torch(logits, 0.8, 0.9, u, occ=b, presence=0.5, count=0.25, decay=0.5)
    assert all(torch.equal(x, y) for x, y in zip(got, want)) and torch.equal(a, b) and not torch.equal(a, occ)
    for bad in (occ[:2], occ.double(), occ[:, :-8]):
        with pytest.raises(ValueError):
            sampling.pick(logits, 0.8, 0.9, u, occ=bad)


# ------------------------------------------------------------------------------------------------ generation
def app_generate(m, ids, images, tau, top_p, n, seed, presence, count, decay, ban, stops=()):
    """forward_stateful step by step, the applications' dict around pick_torch: what generate_stateful must return."""
    from visualrwkv_amd import sampling
    from visualrwkv_amd.rwkv7 import CHUNK_LEN
    samples = {"input_ids": ids, "images": images, "labels": ids}
    u_all = torch.rand(n, 1, generator=gen(seed)).float()
    with torch.no_grad():
        x, _ = m.preparing_embedding(samples)
        rem = x.size(1) % CHUNK_LEN
        x = m.rwkv.pad_left(x, CHUNK_LEN - rem if rem else 0)
        logits, state = m.rwkv.forward_stateful(x, None, last_only=True)
        occurrence, toks, lgs = {}, [], []
        for i in range(n):
            out = logits.clone()
            for t in ban:
                out[0, t] = -math.inf
            for t in occurrence:
                out[0, t] -= float(np.float32(presence) + occurrence[t] * np.float32(count))
            tk, lt, _ = sampling.pick_torch(out, tau, top_p, u_all[i])
            token = int(tk[0])
            toks.append(token)
            lgs.append(float(lt[0]))
            if token in stops:
                break
            for t in occurrence:
                occurrence[t] = np.float32(occurrence[t] * np.float32(decay))
            occurrence[token] = np.float32(occurrence.get(token, np.float32(0)) + np.float32(1))
            logits, state = m.rwkv.forward_stateful(m.rwkv.emb(torch.tensor([[token]])), state, last_only=True)
    return toks, lgs


def test_penalised_generate_stateful_is_the_applications_loop(model):      # noqa: F811
    m, ids, images = model
    plain = m.generate_stateful(ids, images, True, 1.0, 0.0, 2 * N_NEW, -7, generator=gen(3))
    ban = (plain[0][0],)                                     # the unpenalised first token
    for tau, top_p, presence, count in ((1.0, 0.0, 128.0, 0.0), (1.2, 0.9, 0.4, 0.4), (1.0, 0.0, 0.0, 0.0)):
        got = m.generate_stateful(ids, images, True, tau, top_p, 2 * N_NEW, -7, generator=gen(3), presence_penalty=presence,
                                  count_penalty=count, penalty_decay=0.996, token_ban=ban)
        toks, lgs = app_generate(m, ids, images, tau, top_p, 2 * N_NEW, 3, presence, count, 0.996, ban)
        assert got[0] == toks and got[1] == pytest.approx(lgs, rel=1e-12) and ban[0] not in got[0]
        if presence == 128.0:
            assert len(set(got[0])) == len(got[0])           # a presence penalty above every logit gap: no token twice


def test_penalised_generate_reruns(model):      # noqa: F811
    """The re-running generate takes the same arguments: no token twice under a presence penalty of 128 at top_p = 0, the ban holds, and
    the same generator gives the same run."""
    m, ids, images = model
    first = m.generate(ids, images, False, 1.0, 1.0, 1, -7)[0][0]
    a = m.generate(ids, images, True, 1.0, 0.0, N_NEW, -7, generator=gen(4), presence_penalty=128.0, token_ban=[first])
    b = m.generate(ids, images, True, 1.0, 0.0, N_NEW, -7, generator=gen(4), presence_penalty=128.0, token_ban=[first])
    assert a == b and len(set(a[0])) == N_NEW and first not in a[0]


def test_argument_errors(model):      # noqa: F811
    from visualrwkv_amd import sampling
    m, ids, images = model
    l, u = torch.zeros(1, 8), torch.tensor([0.5])
    bad = [dict(presence=-0.1), dict(presence=math.nan), dict(presence=math.inf), dict(count=-1.0), dict(count=math.nan),
           dict(decay=0.0), dict(decay=1.5), dict(decay=-0.5), dict(decay=math.nan)]
    bufs = sampling.PickBuffers(1, "cpu", V=8)
    for kw in bad:
        with pytest.raises(ValueError):
            sampling.pick(l, 1.0, 0.9, u, occ=torch.zeros(1, 8), **kw)
        with pytest.raises(ValueError):
            sampling.pick_torch(l, 1.0, 0.9, u, occ=torch.zeros(1, 8), **kw)
        with pytest.raises(ValueError):
            bufs.set(1.0, 0.9, **{"presence": 0.0, "count": 0.0, "decay": 0.996, **kw})
        names = {"presence": "presence_penalty", "count": "count_penalty", "decay": "penalty_decay"}
        for fn in (m.generate, m.generate_stateful):
            with pytest.raises(ValueError):
                fn(ids, images, True, 1.0, 0.9, 2, -7, **{names[k]: v for k, v in kw.items()})
    for ban in ((-1,), (8,), (3, 1000), (1.5,)):
        with pytest.raises(ValueError):
            bufs.reset(ban)
    for ban in ((-1,), (1000,), (5, 70000)):                 # the model's vocabulary has 1000 tokens
        for fn in (m.generate, m.generate_stateful):
            with pytest.raises(ValueError):
                fn(ids, images, True, 1.0, 0.9, 2, -7, token_ban=ban)
    bufs.reset((0, 7))
    assert bufs.occ.tolist() == [[-1.0, 0, 0, 0, 0, 0, 0, -1.0]]
    for kw in (dict(presence_penalty=0.5), dict(count_penalty=0.5), dict(token_ban=(3,))):      # greedy decoding under penalties: top_p = 0
        for fn in (m.generate, m.generate_stateful):
            with pytest.raises(ValueError):
                fn(ids, images, False, 1.0, 1.0, 2, -7, **kw)


def test_a_stop_list_ends_the_run_at_whichever_comes_first(model):      # noqa: F811
    m, ids, images = model
    for fn in (m.generate, m.generate_stateful):
        for do_sample, kw in ((False, {}), (True, dict(generator=gen(5))), (True, dict(generator=gen(5), presence_penalty=0.5))):
            kw = {k: (gen(5) if k == "generator" else v) for k, v in kw.items()}
            full = fn(ids, images, do_sample, 1.0, 0.9, N_NEW, -7, **kw)
            assert len(full[0]) == N_NEW
            early, late = full[0][2], full[0][4]
            for stop in ([late, early], (early, late), [early], early, {late, early}):
                kw = {k: (gen(5) if k == "generator" else v) for k, v in kw.items()}
                cut = fn(ids, images, do_sample, 1.0, 0.9, N_NEW, stop, **kw)
                n = min(full[0].index(t) for t in ([stop] if isinstance(stop, int) else stop)) + 1
                assert cut[0] == full[0][:n] and cut[1] == full[1][:n], (fn.__name__, do_sample, stop)


def test_default_arguments_change_nothing(model):      # noqa: F811
    m, ids, images = model
    for fn in (m.generate, m.generate_stateful):
        for do_sample in (False, True):
            a = fn(ids, images, do_sample, 1.1, 0.9, N_NEW, -7, generator=gen(6))
            b = fn(ids, images, do_sample, 1.1, 0.9, N_NEW, [-7], generator=gen(6), presence_penalty=0.0, count_penalty=0.0,
                   penalty_decay=0.996, token_ban=())
            assert a == b and len(a[0]) == N_NEW


def test_prototype_counts_the_header_arguments():
    from visualrwkv_amd import hip_lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "visualrwkv_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    args = re.search(r"int\s+vrwkv_sample_pick_pen_bf16\s*\(([^)]*)\)", hdr).group(1).split(",")
    res, argtypes = hip_lib.PROTOTYPES["vrwkv_sample_pick_pen_bf16"]
    assert len(argtypes) == len(args) == 12 and "occ" in args[6] and "stream" in args[-1]
