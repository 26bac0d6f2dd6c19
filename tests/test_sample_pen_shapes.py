"""The penalised sampling head -- csrc/sample_head.hip, vrwkv_sample_pick_pen_bf16 -- through the C ABI, on the two backends of
tests/test_sample_shapes.py with the same test bodies: the host lockstep emulator (CPU tensors, no marker) and the product library (CUDA
tensors, `gpu` marker).

The oracle needs no epsilon.  The contract (include/visualrwkv_hip.h) says that the penalised entry on (l, occ) is the plain entry on the row
l' -- -inf where occ < 0, bf16(l - (alpha_presence + occ alpha_count)) where occ > 0, l elsewhere -- so every launch (run_pen()) makes l' on
the host in torch (fp32 operations, each rounded on its own, one rounding to bf16), runs the PLAIN entry on it through
test_sample_shapes.run (which asserts that entry's own properties), and asserts bit for bit: token, l_token, p_token and x_out of the
penalised call are the plain call's; occ afterwards is the contract's in torch fp32 -- c decay where c > 0, the same bits elsewhere, + 1 at
the token.  That the plain entry agrees with fp64 is test_sample_shapes.py's business.

Every launch: occ is passed as rows 1 .. B of a buffer of B + 2 rows whose first and last row are sentinels (the rows around the ones
exercised keep their bits); token, logit_prob and x_out carry a guard row behind them, sentinel / NaN before and after.

Positions come from edges(V) / spread(V, n) of test_sample_shapes.py: either side of a chunk's, a lane segment's and a wave's edge.  The
emulator walks 1024 fibers per row whatever V is (0.13 s), so on it test_sparse_occ runs three of the six (top_p, temperature) settings (every
value of each), the edge pairs are taken in one order each, and the carried state of three rows at once is left to the MI355X."""
import math

import numpy as np
import pytest
import torch

from tests.test_glue_shapes import I, P, VP, bits, nan_rows
from tests.test_sample_shapes import (EALIGN, EINVAL, ESHAPE, SENT, U_TOP, _params, be, cpt_of, cpu_gen, edges, emb_for,      # noqa: F401  (be: fixture)
                                      peaked, run, spread)

ARGT_PEN = [I, I, I] + [VP] * 8
GUARD = 77.25                                # the rows around occ
DYADIC = dict(ap=0.5, ac=0.25, decay=255.0 / 256.0)      # with dyadic counts every fp32 operation of the contract is exact
PEN_V = [8, 2056, 8200, 65528, 65536]

assert DYADIC["decay"] == 0.99609375


def f32(x):
    return torch.tensor(x, dtype=torch.float32)


def lprime_host(logits, occ, ap, ac):
    """The contract's l' for logits (B, V) bf16 and occ (B, V) fp32 on the CPU: product, sum and difference in fp32, one rounding to bf16."""
    pen = f32(ap) + occ * f32(ac)
    lp = torch.where(occ > 0, (logits.float() - pen).bfloat16(), logits)
    return torch.where(occ < 0, torch.full_like(lp, -math.inf), lp)


def occ_after_host(occ, tk, decay):
    out = torch.where(occ > 0, occ * f32(decay), occ)
    out[torch.arange(occ.size(0)), tk] += 1.0
    return out


def run_pen(be, logits, occ, tau, top_p, u, emb=None, ap=0.5, ac=0.25, decay=255.0 / 256.0):
    """One penalised launch on logits (B, V) bf16 and occ (B, V) fp32 (CPU tensors) against the plain entry on the host-made l' and the
    contract's occ (module docstring).  Returns token, l_token and occ after the call, on the CPU."""
    B, V = logits.shape
    C = emb.shape[1] if emb is not None else 8
    logits, occ = logits.cpu().contiguous(), occ.cpu().contiguous()
    tk, lt, pt = run(be, lprime_host(logits, occ, ap, ac).to(be.dev), tau, top_p, u, emb)
    params = torch.tensor([tau, top_p, ap, ac, decay], dtype=torch.float32, device=be.dev)
    uu = torch.as_tensor(u, dtype=torch.float64).to(torch.float32).to(be.dev).reshape(B).contiguous()
    buf = torch.full((B + 2, V), GUARD, dtype=torch.float32)
    buf[1:B + 1] = occ
    buf = buf.to(be.dev)
    token = torch.full((B + 1,), SENT, dtype=torch.int32, device=be.dev)
    lp = nan_rows(be, B, 2, torch.float32)
    x_out = nan_rows(be, B, C) if emb is not None else None
    rc = be.rc("vrwkv_sample_pick_pen_bf16", ARGT_PEN, B, V, C, P(logits.to(be.dev)), P(params), P(uu), P(buf[1]), P(emb), P(x_out), P(token), P(lp))
    assert rc == 0, rc
    if be.name == "hip":
        torch.cuda.synchronize()
    token, lp, buf = token.cpu(), lp.cpu(), buf.cpu()
    assert int(token[-1]) == SENT and bool(torch.isnan(lp[-1]).all()), "guard row written"
    assert bool((buf[0] == GUARD).all()) and bool((buf[-1] == GUARD).all()), "occ: a row around the exercised ones written"
    assert torch.equal(token[:B].long(), tk), f"tokens {token[:B].tolist()}, the plain entry on l' gives {tk.tolist()}"
    assert torch.equal(bits(lp[:B, 0].contiguous()), bits(lt.contiguous())), "l_token differs from the plain entry's on l'"
    assert torch.equal(bits(lp[:B, 1].contiguous()), bits(pt.contiguous())), "p_token differs from the plain entry's on l'"
    if emb is not None:
        x_out = x_out.cpu()
        assert bool(torch.isnan(x_out[-1].float()).all()), "x_out: guard row written"
        assert torch.equal(bits(x_out[:B]), bits(emb.cpu()[tk])), "x_out != emb[token]"
    want = occ_after_host(occ, tk, decay)
    got = buf[1:B + 1]
    bad = torch.nonzero(bits(got) != bits(want))
    assert bad.numel() == 0, f"occ differs from the contract at {bad[:8].tolist()}: {got[tuple(bad[0])].item()!r} for {want[tuple(bad[0])].item()!r}"
    return tk, lp[:B, 0], got.clone()


def us_for(B):
    return [0.0, 0.5, U_TOP][:B] if B == 3 else [0.5]


# ------------------------------------------------------------------------------------------------ sizes
@pytest.mark.parametrize("backend,V,B,C", _params([(V, B, C) for V in PEN_V for B in (1, 3) for C in (8, None)]))
def test_zero_occ_is_the_plain_pick(backend, be, V, B, C):
    """No token has occurred: the plain entry on l itself; afterwards occ is 1 at each row's token and 0 elsewhere."""
    logits = peaked(300 + V % 89 + B, B, V)
    us = [(0.41 + 0.23 * b) % 1.0 for b in range(B)]
    tk, _, after = run_pen(be, logits, torch.zeros(B, V), 1.3, 0.9, us, emb_for(be, V, C), ap=0.3, ac=0.1, decay=0.996)
    want = torch.zeros(B, V)
    want[torch.arange(B), tk] = 1.0
    assert torch.equal(after, want)


def sparse_case(V, B):
    """Rows whose counted tokens are their likeliest ones: dyadic counts at edges(V), spread(V, 20), spread(V, 5), a banned one among them."""
    logits = peaked(500 + V % 83, B, V).clamp_(-8, 8)
    occ = torch.zeros(B, V)
    counts = [1.0, 2.0, 0.5, 1.5, 3.0, 255.0 / 256.0, 4.0, 0.25]
    for b in range(B):
        pos = [edges(V), spread(V, min(20, V // 2)), spread(V, min(5, V // 2))][b]
        for k, p in enumerate(pos):
            logits[b, p] = 9.0 + 0.5 * (k % 5)
            occ[b, p] = counts[(k + b) % len(counts)]
        occ[b, pos[len(pos) // 2]] = -1.0
    return logits, occ


@pytest.mark.parametrize("backend,V,B", _params([(V, B) for V in PEN_V for B in (1, 3)]))
def test_sparse_occ(backend, be, V, B):
    """Dyadic counts, alpha_presence = 0.5, alpha_count = 0.25, decay = 255/256 at top_p in {0, 0.5, 1}, temperature in {0.7, 1}, u in
    {0, 0.5, 1 - 2^-24} (B = 3: one u per row, every row with its own counts -- the row stride of occ; B = 1: u = 0.5)."""
    logits, occ = sparse_case(V, B)
    emb = emb_for(be, V, 8 if V % 16 == 8 else None)
    settings = [(top_p, tau) for top_p in (0.0, 0.5, 1.0) for tau in (0.7, 1.0)]
    if be.name == "emu":
        settings = [(0.0, 0.7), (0.5, 1.0), (1.0, 0.7)]
    for top_p, tau in settings:
        run_pen(be, logits, occ, tau, top_p, us_for(B), emb, **DYADIC)


# ------------------------------------------------------------------------------------------------ the penalty decides
def edge_pairs(V):
    """(i, j) on either side of a chunk edge, a lane segment's edge and a wave's edge, in both orders."""
    seg = 8 * cpt_of(V)
    pairs = [(a, a + 1) for a in (7, seg - 1, 64 * seg - 1) if a + 1 < V] or [(3, 5)]
    return sorted(set(pairs + [(j, i) for i, j in pairs]))


@pytest.mark.parametrize("backend,V", _params([8, 2056, 8200, 65536]))
def test_the_penalty_changes_the_winner(backend, be, V):
    """top_p = 0.  The maximum 8 at i, the runner-up 7 at j, four rows in one launch: with no count i wins; a count of 4 at i (penalty 1.5)
    makes j the token; a count of 2 (penalty 1) a tie that keeps both, in index order (u = 0.25 and 0.75).  The emulator takes each edge in
    one order only."""
    base = torch.randn(V, generator=cpu_gen(13)).clamp_(-3, 3)
    pairs = edge_pairs(V)
    if be.name == "emu":
        pairs = [pr for pr in pairs if pr[0] < pr[1]][-2 if V == 65536 else None:]
        pairs = [pr if n % 2 else pr[::-1] for n, pr in enumerate(pairs)]
    for i, j in pairs:
        row = base.clone()
        row[i], row[j] = 8.0, 7.0
        logits = row.bfloat16().view(1, V).repeat(4, 1)
        occ = torch.zeros(4, V)
        occ[1, i], occ[2, i], occ[3, i] = 4.0, 2.0, 2.0
        tk, lt, _ = run_pen(be, logits, occ, 1.0, 0.0, [0.5, 0.5, 0.25, 0.75], **DYADIC)
        assert tk.tolist() == [i, j, min(i, j), max(i, j)] and lt.tolist() == [8.0, 7.0, 7.0, 7.0], (i, j)


@pytest.mark.parametrize("backend,V", _params([8, 2056]))
def test_bf16_rounding_of_the_penalised_logit(backend, be, V):
    """l' is rounded to bf16, to nearest even, read back through l_token: 1 - 2^-9 -> 1 and 1 - 3 2^-9 -> 0.9921875 (both ties),
    1 - 2^-8 -> 0.99609375; -inf under a count stays -inf and is never the token."""
    at = edges(V)[-2]
    for pen, want in ((2.0 ** -9, 1.0), (3 * 2.0 ** -9, 0.9921875), (2.0 ** -8, 0.99609375)):
        row = torch.full((V,), -6.0)
        row[at] = 1.0
        occ = torch.zeros(1, V)
        occ[0, at] = 1.0
        tk, lt, _ = run_pen(be, row.bfloat16().view(1, V), occ, 1.0, 0.0, [0.5], ap=pen, ac=0.0, decay=0.5)
        assert tk.tolist() == [at] and lt.tolist() == [want]
    row = torch.full((V,), 2.0)
    row[0] = row[at] = -math.inf
    occ = torch.zeros(1, V)
    occ[0, 0] = occ[0, at] = 3.0
    assert bool(torch.isinf(lprime_host(row.bfloat16().view(1, V), occ, 0.5, 0.25)[0, [0, at]]).all())
    tk, _, after = run_pen(be, row.bfloat16().view(1, V), occ, 1.0, 1.0, [0.0], **DYADIC)
    assert tk.tolist() == [1] and float(after[0, 0]) == 3.0 * 255 / 256


# ------------------------------------------------------------------------------------------------ ban
@pytest.mark.parametrize("backend,V", _params([8, 2056, 65528]))
def test_ban(backend, be, V):
    """The maximum is banned and the next one wins, call after call; the banned entries -- one of them in the last live chunk -- keep their
    -1 bits through 3 calls on the carried occ."""
    row = torch.randn(V, generator=cpu_gen(17)).clamp_(-3, 3)
    top, nxt = V - 3, edges(V)[len(edges(V)) // 2]
    row[top], row[nxt] = 9.0, 8.0
    banned = sorted({top, 0, V - 8})
    logits = row.bfloat16().view(1, V)
    occ = torch.zeros(1, V)
    occ[0, banned] = -1.0
    minus_one = bits(torch.tensor([-1.0]))
    for call in range(3):
        tk, lt, occ = run_pen(be, logits, occ, 1.0, 0.0, [0.5], emb_for(be, V, 8), ap=0.25, ac=0.125, decay=0.5)
        assert tk.tolist() == [nxt] and lt.tolist() == [8.0 - (0.0 if call == 0 else 0.25 + 0.125 * (2.0 - 0.5 ** (call - 1)))]
        assert bool((bits(occ[0, banned]) == minus_one).all())
    tk, _, _ = run_pen(be, logits, occ, 1.0, 1.0, [0.0], **DYADIC)      # every token is in K, index 0 is banned: the first with weight is 1
    assert tk.tolist() == [1]


# ------------------------------------------------------------------------------------------------ carried state
def app_loop(row, n, ap, ac, decay):
    """The applications' loop (v7.10/app/app_gpu.py:56-86) with a dict, in fp32, at top_p = 0: tokens and the dict after every pick."""
    ap, ac, decay = np.float32(ap), np.float32(ac), np.float32(decay)
    occurrence, steps = {}, []
    for _ in range(n):
        out = row.clone()                                    # bf16
        for t in occurrence:
            out[t] = float(np.float32(float(out[t])) - (ap + occurrence[t] * ac))      # rounded to bf16 by the assignment
        top = out.float().max()
        assert int((out.float() == top).sum()) == 1, "the carried-state row must have no tie"
        token = int(out.float().argmax())
        for t in occurrence:
            occurrence[t] = np.float32(occurrence[t] * decay)
        occurrence[token] = np.float32(occurrence.get(token, np.float32(0)) + np.float32(1))
        steps.append((token, dict(occurrence)))
    return steps


@pytest.mark.parametrize("backend,V,B", _params([(2056, 1)]) + [c for c in _params([(8200, 3)]) if c.id.startswith("hip")])
def test_carried_state(backend, be, V, B):
    """6 calls on carried counts at top_p = 0 with a count penalty that rotates the winner among the likeliest tokens: tokens and occ after
    every call are the applications' dict loop's."""
    logits = peaked(700 + B, B, V).clamp_(-4, 4)
    for b in range(B):
        for k, p in enumerate(spread(V, 3 + b)):
            logits[b, p] = 9.0 - 0.5 * k
    ap, ac, decay = 0.25, 1.5, 0.996
    want = [app_loop(logits[b], 6, ap, ac, decay) for b in range(B)]
    assert all(len({t for t, _ in w}) >= 3 for w in want), "the winner does not rotate"
    occ = torch.zeros(B, V)
    for call in range(6):
        tk, _, occ = run_pen(be, logits, occ, 1.0, 0.0, [0.5] * B, ap=ap, ac=ac, decay=decay)
        for b in range(B):
            token, d = want[b][call]
            assert int(tk[b]) == token, (call, b)
            ref = torch.zeros(V)
            for t, c in d.items():
                ref[t] = float(c)
            assert torch.equal(bits(occ[b]), bits(ref)), (call, b)


# ------------------------------------------------------------------------------------------------ random rows
def clear_of_midpoints(logits, occ, ap, ac):
    """In fp64: no penalised element's exact l - (alpha_presence + c alpha_count) lies within 4 fp32 ulp of max(|l|, pen) of a midpoint between
    two bf16 values -- then neither the rounding of the fp32 operations nor a contracted multiply-add can change the bf16 result."""
    on = occ > 0
    l = logits.double()[on]
    pen = f32(ap).double() + occ.double()[on] * f32(ac).double()
    x = l - pen
    ulp16 = torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(1e-30))) - 7)
    frac = x.abs() / ulp16
    dist = ((frac - torch.floor(frac)) - 0.5).abs() * ulp16
    ulp32 = torch.exp2(torch.floor(torch.log2(torch.maximum(l.abs(), pen).clamp_min(1e-30))) - 23)
    return bool((dist > 4 * ulp32).all())


def random_case(V, B):
    for attempt in range(64):
        g = cpu_gen(9000 + V % 71 + attempt)
        logits = (6 * torch.randn(B, V, generator=g)).bfloat16()
        occ = torch.zeros(B, V)
        n = min(V, 192)
        for b in range(B):
            pos = torch.randperm(V, generator=g)[:n]
            occ[b, pos] = (5 * torch.rand(n, generator=g)).float() + 2.0 ** -10
            top = logits[b].float().topk(min(V, 8)).indices          # the likeliest tokens have occurred
            occ[b, top] = (3 * torch.rand(top.numel(), generator=g)).float() + 0.5
        if clear_of_midpoints(logits, occ, 0.3, 0.1):
            return logits, occ, attempt
    raise AssertionError("no seed of 64 keeps every penalised element clear of the bf16 rounding midpoints")


@pytest.mark.parametrize("backend,V,B", _params([(8, 3), (2056, 3), (65536, 2)]))
def test_random_rows(backend, be, V, B):
    """decay = 0.996, alpha_presence = 0.3, alpha_count = 0.1, random counts: the same differential assertion, after the host has made sure
    in fp64 that no rounding midpoint is near (clear_of_midpoints)."""
    logits, occ, _ = random_case(V, B)
    us = torch.rand(B, generator=cpu_gen(31), dtype=torch.float64).tolist()
    for top_p, tau in ((0.9, 0.9), (0.3, 1.0)):
        run_pen(be, logits, occ, tau, top_p, us, emb_for(be, V, 8), ap=0.3, ac=0.1, decay=0.996)


# ------------------------------------------------------------------------------------------------ rejections
def _reject_setup(be):
    B, V, C = 2, 64, 16
    t = {
        "logits": torch.zeros(B * V + 8, dtype=torch.bfloat16, device=be.dev),
        "params": torch.tensor([2.0, 0.5, 0.5, 0.25, 0.5, 1.0], dtype=torch.float32, device=be.dev),
        "u": torch.full((B + 2,), 0.5, dtype=torch.float32, device=be.dev),
        "occ": torch.full(((B + 1) * V,), 2.0, dtype=torch.float32, device=be.dev),
        "emb": torch.zeros(V + 1, C, dtype=torch.bfloat16, device=be.dev),
        "x_out": nan_rows(be, B + 1, C),
        "token": torch.full((B + 2,), SENT, dtype=torch.int32, device=be.dev),
        "logit_prob": nan_rows(be, B + 1, 2, torch.float32),
    }
    return B, V, C, t


ORDER = ("logits", "params", "u", "occ", "emb", "x_out", "token", "logit_prob")
REJECTS = [
    # id                     sizes (B, V, C)     NULL            moved off its alignment    code
    ("null:occ",             (2, 64, 16),        ("occ",),       (),                        EINVAL),
    ("off:occ",              (2, 64, 16),        (),             ("occ",),                  EALIGN),
    ("null:logits",          (2, 64, 16),        ("logits",),    (),                        EINVAL),
    ("off:params",           (2, 64, 16),        (),             ("params",),               EALIGN),
    # two faults: what the plain entry's order gives -- the count, the shape, NULL, the alignment
    ("B0 + null:occ",        (0, 64, 16),        ("occ",),       (),                        EINVAL),
    ("V12 + null:occ",       (2, 12, 16),        ("occ",),       (),                        ESHAPE),
    ("C12 + off:occ",        (2, 64, 12),        (),             ("occ",),                  ESHAPE),
    ("null:occ + off:logits", (2, 64, 16),       ("occ",),       ("logits",),               EINVAL),
    ("null:u + off:occ",     (2, 64, 16),        ("u",),         ("occ",),                  EINVAL),
]


@pytest.mark.parametrize("backend,case", _params([r[0] for r in REJECTS]))
def test_rejects(backend, be, case):
    """The exact code; a refused call writes nothing.  Off its alignment: occ by 4 bytes (an element, not a 16-byte piece), the rest by 2."""
    _, sizes, nulls, offs, code = next(r for r in REJECTS if r[0] == case)
    _, _, _, t = _reject_setup(be)
    ptr = {name: None if name in nulls else VP(buf.data_ptr() + (4 if name == "occ" else 2)) if name in offs else P(buf) for name, buf in t.items()}
    before = {name: buf.clone() for name, buf in t.items()}
    rc = be.rc("vrwkv_sample_pick_pen_bf16", ARGT_PEN, *sizes, *(ptr[n] for n in ORDER))
    if be.name == "hip":
        torch.cuda.synchronize()
    assert rc == code, (case, rc)
    for name, buf in t.items():
        assert torch.equal(bits(buf), bits(before[name])), f"{name} written"


@pytest.mark.parametrize("backend", _params([()]))
def test_accepts_the_valid_call(backend, be):
    """The setup the rejections start from is itself accepted, with and without the embedding."""
    B, V, C, t = _reject_setup(be)
    args = lambda **kw: [kw.get(n, P(t[n])) for n in ORDER]      # noqa: E731
    assert be.rc("vrwkv_sample_pick_pen_bf16", ARGT_PEN, B, V, C, *args()) == 0
    assert be.rc("vrwkv_sample_pick_pen_bf16", ARGT_PEN, B, V, C, *args(emb=None, x_out=None)) == 0
    if be.name == "hip":
        torch.cuda.synchronize()
    assert int(t["token"][-1]) == SENT and bool(torch.isnan(t["x_out"][B:].float()).all())
    assert bool((t["occ"][B * V:] == 2.0).all()), "occ written past its B rows"
