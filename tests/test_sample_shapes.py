"""The sampling head of the decode step -- csrc/sample_head.hip, vrwkv_sample_pick_bf16 -- through the C ABI, on two backends with the same
test bodies: the host lockstep emulator (tests/emu/emu_sample_head.cpp compiles the .hip file whole: CPU tensors, no marker) and the
product library (CUDA tensors, `gpu` marker).

The oracle (class Ref) is the contract of include/visualrwkv_hip.h in fp64 torch, one row at a time: p = softmax(l); the nucleus K = every
token whose logit is at least that of the first token, in descending order, at which the running sum of p reaches top_p (top_p >= 1: all);
q = exp((l - max l) / temperature) on K; the normalised running sum of q over K in index order is the CDF, and u picks the first member
whose CDF value exceeds it (the last member of weight > 0 if none does).  It is not sampling.pick_torch.

Every launch (run()) asserts: return code 0; token is a sentinel and logit_prob / x_out are NaN before the call, each with a guard row
behind it -- results written and in range, guards untouched; x_out == emb[token] bit for bit; l_token == the row's bf16 value at token,
exactly; a second call on the same inputs is bit-identical.

What picks the kernel's path is V alone: 1024 threads, thread t owns the cpt = ceil(V / 8 / 1024) chunks of 8 elements from chunk t cpt on
(SAMPLE_V says what every width reaches).  A segment is 8 cpt elements, a wave's 512 cpt: edges() lists the indices on either side of a
chunk, a lane's segment and a wave's, which the exact cases use as positions.

epsilon.  The kernel compares fp32 sums: a mass or a prefix is at most 8 cpt <= 64 terms per thread in sequence, 6 butterfly levels, 16 wave
partials in sequence (the scan: 63 lanes, then 15 waves, then the walk's 64), i.e. at most 64 + 63 + 15 + 1 = 143 roundings of relative size
2^-24 on a prefix and 64 + 6 + 15 = 85 on a total; every term carries the 1 ulp of v_exp_f32 and half an ulp each of the subtraction l - max l
and the fraction of the split exponent (exp2_scaled), 2 ulp together.  A comparison of a prefix against u total therefore moves by at most
(143 + 2) + (85 + 2) + 1 (the product) = 233 ulp, the cut's comparison of a mass against top_p Z by (85 + 2) 2 + 1 = 175: both below
EPS = 2^-15 = 512 2^-24, which is what the tests use (asserted below from these counts).  Where u lies within EPS of a CDF boundary the
neighbour across it is accepted too; the share of such cases is computed on the fp64 reference alone and asserted to stay below 1 %
(the random rows: 0 of 1152 cases at V = 2056, 1 of 768 = 0.13 % at V = 65 536).  The random rows assert, in fp64 and unskipped, that no level's
cumulative mass lies within EPS of top_p, and that |K| <= 128.

p_token.  |got - fp64| <= p_token (n_terms + 4) 2^-24 with n_terms = 8 cpt + 6 + 16 (the roundings of Z) -- every case, the decoy included that u = 0 at
top_p = 1 picks in front of a needle 43 above it (p_token near 1e-19, a normal fp32; its exponent is formed exactly: exp2_scaled).  Worst ratio to the bound: 0.094 on the emulator and 0.094 on the MI355X (both: the ties case at V = 65 536;
the random rows stay below 0.04), so the hardware exp needs no wider bound.
VRWKV_TEST_NOTES=1 prints the figures.
"""
import ctypes
import math

import pytest
import torch

from tests.parity import NOTES
from tests.test_glue_shapes import I, P, VP, Backend, bits, nan_rows

EINVAL, ESHAPE, EALIGN = -1, -2, -3
BACKENDS = ["emu", pytest.param("hip", marks=pytest.mark.gpu)]
ARGT = [I, I, I] + [VP] * 7
THREADS, MAX_V = 1024, 65536
EPS = 2.0 ** -15
SENT = -7                                   # token before the call
U_TOP = 1.0 - 2.0 ** -24                    # the largest fp32 below 1
WORST = {}

assert (64 + 63 + 15 + 1 + 2) + (64 + 6 + 15 + 2) + 1 <= EPS * 2 ** 24 and 2 * (64 + 6 + 15 + 2) + 1 <= EPS * 2 ** 24       # module docstring

#            V      what it reaches
SAMPLE_V = [
    (8,      "one chunk: one live thread"),
    (2040,   "255 threads: the last lane of wave 3 idle"),
    (2048,   "four full waves"),
    (2056,   "one live lane in wave 4"),
    (4104,   "513 threads"),
    (8192,   "cpt = 1 full: every thread one chunk"),
    (8200,   "cpt = 2: thread 512 owns the last chunk and a dead one, 511 threads idle"),
    (16384,  "cpt = 2 full"),
    (16392,  "cpt = 3"),
    (57344,  "cpt = 7 full"),
    (57352,  "cpt = 8: the widest segment, 128 threads idle"),
    (65528,  "cpt = 8, the last thread's last chunk dead"),
    (65536,  "the cap: 128 KB of keys in LDS, 64 elements per thread"),
]
SAMPLE_C = (8, 2040, 2048, 2056, None)      # None: emb = x_out = NULL


def _params(items):
    out = []
    for b in BACKENDS:
        name, marks = (b, ()) if isinstance(b, str) else (b.values[0], b.marks)
        for it in items:
            it = it if isinstance(it, tuple) else (it,)
            out.append(pytest.param(name, *it, id="-".join(str(v) for v in (name,) + it), marks=marks))
    return out


@pytest.fixture
def be(request, backend):
    return Backend(request, backend)


def cpt_of(V):
    return -(-(V // 8) // THREADS)


def n_terms(V):
    return 8 * cpt_of(V) + 6 + 16


def edges(V):
    """Indices on either side of a chunk's, a lane's segment's and a wave's edge, the row's ends."""
    seg = 8 * cpt_of(V)
    cand = [0, 7, 8, 63, 64, seg - 1, seg, 64 * seg - 1, 64 * seg, V // 2 - 1, V // 2, V - 8, V - 1]
    return sorted({i for i in cand if 0 <= i < V})


def spread(V, n):
    """n distinct positions: the edges first, then evenly spaced odd ones."""
    pos = edges(V)[:n] if n <= len(edges(V)) else list(edges(V))
    i = 0
    while len(pos) < n:
        c = (i * (V // (n + 1)) + 3) % V
        i += 1
        if c not in pos:
            pos.append(c)
    return sorted(pos)


class Ref:
    """One row of the contract in fp64."""
    def __init__(self, row, tau, top_p):
        l = row.detach().cpu().double()
        self.l, self.V = l, l.numel()
        m = l.max()
        e = torch.exp(l - m)
        self.p = e / e.sum()
        ls, order = torch.sort(l, descending=True, stable=True)
        cum = torch.cumsum(self.p[order], 0)
        self.levels = cum[torch.cat((ls[1:] != ls[:-1], torch.tensor([True])))]       # cumulative mass at the end of every level
        if top_p >= 1:
            self.K = torch.ones_like(l, dtype=torch.bool)
        else:
            reach = torch.nonzero(cum >= top_p)
            self.K = l >= ls[int(reach[0]) if reach.numel() else self.V - 1]
        q = torch.where(self.K, torch.exp((l - m) / tau), torch.zeros_like(l))
        self.members = torch.nonzero(q > 0).view(-1)
        self.cdf = torch.cumsum(q[self.members], 0) / q.sum()

    def clear_of_cut(self, top_p):
        return top_p >= 1 or top_p <= 0 or bool(((self.levels - top_p).abs() > EPS).all())

    def token(self, u):
        u = torch.as_tensor(u, dtype=torch.float64).view(-1)
        j = torch.searchsorted(self.cdf, u, right=True).clamp_(max=self.members.numel() - 1)
        return self.members[j]

    def accepted(self, u):
        """Per u: the member positions [j0, j1] whose CDF interval, widened by EPS, holds u."""
        u = torch.as_tensor(u, dtype=torch.float64).view(-1)
        n = self.members.numel()
        j0 = torch.searchsorted(self.cdf, u - EPS, right=True).clamp_(max=n - 1)
        j1 = torch.searchsorted(self.cdf, u + EPS, right=True).clamp_(max=n - 1)
        return j0, j1

    def clear_of_cdf(self, u):
        u = torch.as_tensor(u, dtype=torch.float64).view(-1, 1)
        return bool(((self.cdf.view(1, -1) - u).abs() > EPS).all())


def run(be, logits, tau, top_p, u, emb=None):
    """Two launches on fresh outputs; the assertions every case shares (module docstring).  Returns token, l_token, p_token on the CPU."""
    B, V = logits.shape
    C = emb.shape[1] if emb is not None else 8
    params = torch.tensor([tau, top_p], dtype=torch.float32, device=be.dev)
    u = torch.as_tensor(u, dtype=torch.float64).to(torch.float32).to(be.dev).reshape(B).contiguous()
    outs = []
    for _ in range(2):
        token = torch.full((B + 1,), SENT, dtype=torch.int32, device=be.dev)
        lp = nan_rows(be, B, 2, torch.float32)
        x_out = nan_rows(be, B, C) if emb is not None else None
        rc = be.rc("vrwkv_sample_pick_bf16", ARGT, B, V, C, P(logits), P(params), P(u), P(emb), P(x_out), P(token), P(lp))
        assert rc == 0, rc
        if be.name == "hip":
            torch.cuda.synchronize()
        outs.append((token.cpu(), lp.cpu(), x_out.cpu() if x_out is not None else None))
    (token, lp, x_out), (token2, lp2, x_out2) = outs
    assert int(token[-1]) == SENT and bool(torch.isnan(lp[-1]).all()), "guard row written"
    assert bool(((token[:B] >= 0) & (token[:B] < V)).all()), f"token out of range: {token[:B].tolist()}"
    assert bool(torch.isfinite(lp[:B]).all()), "logit_prob: not written"
    assert torch.equal(token, token2) and torch.equal(bits(lp[:B]), bits(lp2[:B])), "the second call differs"
    tk = token[:B].long()
    if emb is not None:
        assert bool(torch.isnan(x_out[-1].float()).all()), "x_out: guard row written"
        assert torch.equal(bits(x_out[:B]), bits(emb.cpu()[tk])), "x_out != emb[token]"
        assert torch.equal(bits(x_out[:B]), bits(x_out2[:B])), "x_out: the second call differs"
    lrow = logits.cpu().float()
    assert torch.equal(lp[:B, 0], lrow[torch.arange(B), tk]), "l_token is not the row's value at token"
    return tk, lp[:B, 0], lp[:B, 1]


def check_p(be, V, ref, tk, pt, name):
    want = ref.p[tk]
    bound = want * (n_terms(V) + 4) * 2.0 ** -24
    ratio = float(((pt.double() - want).abs() / bound).max())
    key = be.name
    if ratio > WORST.get(key, (0.0, ""))[0]:
        WORST[key] = (ratio, name)
    if NOTES:
        print(f"[sample] {be.name} {name}: p_token worst ratio to its bound {ratio:.3f}   (worst so far {WORST[key][0]:.3f} {WORST[key][1]})")
    assert ratio <= 1.0, f"{name}: p_token off by {ratio:.2f} x its bound"


def one_row(be, row, tau, top_p, us, emb=None, name="", exact=True):
    """One row against every u of `us` in one launch (the row repeated per batch row).  exact: the oracle's token, no tolerance."""
    V = row.numel()
    ref = Ref(row, tau, top_p)
    logits = row.view(1, V).repeat(len(us), 1).contiguous()
    tk, lt, pt = run(be, logits, tau, top_p, us, emb)
    want = ref.token(us)
    if exact:
        assert torch.equal(tk, want), f"{name}: tokens {tk.tolist()} for u {list(us)}, the contract gives {want.tolist()}"
    check_p(be, V, ref, tk, pt, name)
    return ref, tk


def emb_for(be, V, C, seed=5):
    if C is None:
        return None
    return torch.randn(V, C, generator=cpu_gen(seed)).bfloat16().to(be.dev)


def cpu_gen(seed):
    return torch.Generator().manual_seed(seed)       # every input is drawn on the CPU: both backends see the same rows


def peaked(seed, B, V):
    return (6 * torch.randn(B, V, generator=cpu_gen(seed))).bfloat16()


# ------------------------------------------------------------------------------------------------ sizes
SIZE_CASES = [(V, B, SAMPLE_C[(i + j) % len(SAMPLE_C)]) for i, (V, _) in enumerate(SAMPLE_V) for j, B in enumerate((1, 3, 4))
              if V <= 8200 or B != 3 or V == MAX_V]


@pytest.mark.parametrize("backend,V,B,C", _params(SIZE_CASES))
def test_sizes(backend, be, V, B, C):
    """Differing rows and a differing u per batch row at every width of SAMPLE_V; the token is the oracle's or, within EPS of a CDF boundary,
    its neighbour's."""
    if be.name == "emu" and V > 16392 and B == 4 and V != MAX_V:
        B = 2                                    # the emulator walks 1024 fibers per row
    tau, top_p = 1.3, 0.9
    logits = peaked(100 + V % 97 + B, B, V).to(be.dev)
    us = [(0.37 + 0.29 * b) % 1.0 for b in range(B)]
    tk, lt, pt = run(be, logits, tau, top_p, us, emb_for(be, V, C))
    for b in range(B):
        ref = Ref(logits[b], tau, top_p)
        assert ref.clear_of_cut(top_p)
        j0, j1 = ref.accepted(us[b])
        ok = ref.members[int(j0):int(j1) + 1]
        assert int(tk[b]) in ok.tolist(), f"row {b}: token {int(tk[b])}, the contract gives {ref.token(us[b]).tolist()}"
        check_p(be, V, ref, tk[b:b + 1], pt[b:b + 1], f"sizes V{V} B{B} row {b}")


# ------------------------------------------------------------------------------------------------ exact cases
EXACT_V = [8, 2056, 8200, 65536]


@pytest.mark.parametrize("backend,V", _params(EXACT_V))
def test_needle(backend, be, V):
    """One logit 40 above the rest: picked for every u and top_p -- but for u = 0 at top_p = 1 with the needle not in front, where step 4 of
    the contract gives index 0 (the first member of positive weight: its prefix already exceeds u sum q = 0), in fp64 as in the kernel."""
    us = [0.0, 0.5, U_TOP]
    base = torch.randn(V, generator=cpu_gen(7)).clamp_(-3, 3).to(be.dev)
    seg = 8 * cpt_of(V)
    pos = edges(V) if be.name == "hip" else sorted({0, 7 % V, 8 % V, seg - 1, seg % V, V - 1})      # the emulator costs 0.15 s per row
    emb = emb_for(be, V, 8)
    for at in pos:
        row = base.clone()
        row[at] = 43.0
        row = row.bfloat16()
        for top_p in (0.0, 0.5, 1.0):
            ref, tk = one_row(be, row, 1.0, top_p, us, emb if top_p == 0.5 else None, name=f"needle V{V}@{at} top_p {top_p}")
            want = [at, at, at] if top_p < 1 or at == 0 else [0, at, at]
            assert tk.tolist() == want, (at, top_p, tk.tolist())


@pytest.mark.parametrize("backend,V,n", _params([(8, 2), (8, 3), (2056, 2), (2056, 3), (2056, 64), (2056, 65), (8200, 65), (65536, 3), (65536, 65)]))
def test_flat_nucleus(backend, be, V, n):
    """n tokens at one level, the rest 30 below, top_p = 0.9: u = (j + 1/2) / n gives the j-th of them at every temperature -- the prefix in
    index order across chunk, lane and wave edges; u = 1 - 2^-24 stays inside K."""
    pos = spread(V, n)
    row = torch.full((V,), -26.0, device=be.dev)
    row[pos] = 4.0
    row = row.bfloat16()
    js = list(range(n)) if be.name == "hip" else sorted({0, 1, n // 2 - 1, n // 2, n - 2, n - 1})
    us = [(j + 0.5) / n for j in js] + [U_TOP]
    for tau in (0.5, 1.0, 2.0):
        ref, tk = one_row(be, row, tau, 0.9, us, name=f"flat V{V} n{n} tau {tau}")
        assert ref.members.tolist() == pos
        assert tk.tolist() == [pos[j] for j in js] + [pos[-1]]


@pytest.mark.parametrize("backend,V", _params([2056, 65536]))
def test_ties_at_the_cut(backend, be, V):
    """Level 1 alone is below top_p, level 1 and a part of level 2 reach it: K is all of both.  Every member of level 2 is reached, none of
    level 3."""
    l1, l2 = spread(V, 13)[:2], spread(V, 13)[2:8]
    row = torch.full((V,), -5.0 if V == 2056 else -9.0, device=be.dev)
    row[l1], row[l2] = 10.0, 9.0
    row = row.bfloat16()
    top_p = 0.6
    ref = Ref(row, 1.0, top_p)
    assert float(ref.levels[0]) < top_p - EPS and float(ref.p[l1].sum() + ref.p[l2[:1]].sum()) < top_p < float(ref.levels[1]) - EPS
    assert sorted(ref.members.tolist()) == sorted(l1 + l2)
    n = 64 if be.name == "hip" else 16
    us = [(i + 0.5) / n for i in range(n)]
    assert ref.clear_of_cdf(us)
    _, tk = one_row(be, row, 1.0, top_p, us, name=f"ties V{V}")
    assert set(l2) <= set(tk.tolist()) <= set(l1 + l2)


@pytest.mark.parametrize("backend,V,tau", _params([(2056, 0.5), (2056, 2.0), (65536, 0.5), (65536, 2.0)]))
def test_temperature(backend, be, V, tau):
    """K = two levels at distance d = 1: the share of a u grid that lands on level 1 follows exp(d / tau) through the fp64 intervals."""
    pos = spread(V, 8)
    l1, l2 = pos[0::3], [p for p in pos if p not in pos[0::3]]
    row = torch.full((V,), -28.0, device=be.dev)
    row[l1], row[l2] = 2.0, 1.0
    row = row.bfloat16()
    ref = Ref(row, tau, 0.99)
    assert sorted(ref.members.tolist()) == pos
    n = 64 if be.name == "hip" else 16
    us = [(i + 0.5) / n for i in range(n)]
    assert ref.clear_of_cdf(us)
    _, tk = one_row(be, row, tau, 0.99, us, name=f"temperature V{V} tau {tau}")
    share = sum(t in l1 for t in tk.tolist()) / n
    want = len(l1) / (len(l1) + len(l2) * math.exp(-1.0 / tau))
    assert abs(share - want) <= len(pos) / n, (share, want)


@pytest.mark.parametrize("backend", BACKENDS)
def test_top_p_ends(backend, be):
    """top_p = 0: the maximum and its ties, in index order.  top_p = 1 and 1.5: every index of a flat row is reached by its u."""
    for V, at in ((8, (2, 5)), (2056, (63, 2048))):
        row = torch.randn(V, generator=cpu_gen(3)).clamp_(-3, 3).to(be.dev)
        row[list(at)] = 6.0
        _, tk = one_row(be, row.bfloat16(), 1.0, 0.0, [0.0, 0.25, 0.49, 0.51, 0.75, U_TOP], name=f"top_p 0 V{V}")
        assert tk.tolist() == [at[0]] * 3 + [at[1]] * 3
    for V in (8, 2056):
        row = torch.full((V,), 1.5, device=be.dev).bfloat16()
        idx = list(range(V)) if V == 8 or be.name == "hip" else sorted(set(range(0, V, 257)) | {7, 8, 63, 64, 2047, 2048, V - 1})
        for top_p in (1.0, 1.5):
            _, tk = one_row(be, row, 0.7, top_p, [(i + 0.5) / V for i in idx], emb_for(be, V, 16), name=f"flat row V{V} top_p {top_p}")
            assert tk.tolist() == idx


@pytest.mark.parametrize("backend,V", _params([8, 2056, 65536]))
def test_minus_inf(backend, be, V):
    """-inf entries (index 0 and V - 1 among them) are never picked; u = 0 skips a leading -inf."""
    row = torch.randn(V, generator=cpu_gen(11)).to(be.dev)
    holes = sorted({0, 1, V - 1, V // 2, 7 % V})
    row[holes] = -math.inf
    row = row.bfloat16()
    n = 16 if be.name == "hip" else 5
    us = [0.0] + [(i + 0.5) / n for i in range(n)] + [U_TOP]
    first = next(i for i in range(V) if i not in holes)
    for top_p in (1.0, 0.9):
        ref = Ref(row, 1.0, top_p)
        tk, lt, pt = run(be, row.view(1, V).repeat(len(us), 1).contiguous(), 1.0, top_p, us)
        assert not set(tk.tolist()) & set(holes)
        j0, j1 = ref.accepted(us)
        for b in range(len(us)):
            assert int(tk[b]) in ref.members[int(j0[b]):int(j1[b]) + 1].tolist()
        if top_p == 1.0:
            assert int(tk[0]) == first


# ------------------------------------------------------------------------------------------------ random rows
RANDOM_SEEDS = {2056: (0, 1, 2), 65536: (0, 1)}
RANDOM_STATS = {}


@pytest.mark.parametrize("backend,V", _params([2056, 65536]))
def test_random_rows(backend, be, V):
    """Peaked rows l = bf16(6 randn): each (row, u) gives the fp64 oracle's token, or its neighbour across a CDF boundary within EPS of u --
    at most 1 % of the cases, counted on the fp64 reference alone."""
    nu = 64 if be.name == "hip" else 4
    cases = near = 0
    for seed in RANDOM_SEEDS[V] if be.name == "hip" else RANDOM_SEEDS[V][:1]:
        row = peaked(seed, 1, V)[0].to(be.dev)
        us = torch.rand(64, generator=cpu_gen(1000 + seed), dtype=torch.float64)[:nu].tolist()
        for top_p in (0.3, 0.9):
            for tau in (0.7, 1.0, 1.3):
                ref = Ref(row, tau, top_p)
                assert ref.clear_of_cut(top_p), f"seed {seed}: a level's cumulative mass lies within EPS of top_p {top_p}: replace the seed"
                assert int(ref.K.sum()) <= 128
                tk, lt, pt = run(be, row.view(1, V).repeat(nu, 1).contiguous(), tau, top_p, us)
                j0, j1 = ref.accepted(us)
                want = ref.token(us)
                for b in range(nu):
                    ok = ref.members[int(j0[b]):int(j1[b]) + 1].tolist()
                    assert int(tk[b]) in ok, f"seed {seed} top_p {top_p} tau {tau} u {us[b]}: {int(tk[b])}, the contract gives {int(want[b])}"
                cases += nu
                near += int((j1 > j0).sum())
                check_p(be, V, ref, tk, pt, f"random V{V} seed {seed} top_p {top_p} tau {tau}")
    if NOTES:
        print(f"[sample] {be.name} V{V}: {near} of {cases} cases within EPS of a CDF boundary")
    assert near <= 0.01 * cases or be.name == "emu", (near, cases)       # the emulator's few cases: test_random_rows_reference_share counts them all


@pytest.mark.parametrize("V", [2056, 65536])
def test_random_rows_reference_share(V):
    """The share of (row, u) cases within EPS of a CDF boundary, on the fp64 reference alone with all 64 u of every row: at most 1 %."""
    cases = near = 0
    for seed in RANDOM_SEEDS[V]:
        row = peaked(seed, 1, V)[0]
        us = torch.rand(64, generator=cpu_gen(1000 + seed), dtype=torch.float64).tolist()
        for top_p in (0.3, 0.9):
            for tau in (0.7, 1.0, 1.3):
                ref = Ref(row, tau, top_p)
                assert ref.clear_of_cut(top_p) and int(ref.K.sum()) <= 128
                j0, j1 = ref.accepted(us)
                cases += 64
                near += int((j1 > j0).sum())
    assert near <= 0.01 * cases, (near, cases)


# ------------------------------------------------------------------------------------------------ rejections
def _reject_setup(be):
    B, V, C = 2, 64, 16
    t = {
        "logits": torch.zeros(B * (MAX_V + 8) + 8, dtype=torch.bfloat16, device=be.dev),      # wide enough for the width over the cap
        "params": torch.tensor([2.0, 0.5, 1.0, 0.9], dtype=torch.float32, device=be.dev),
        "u": torch.full((B + 2,), 0.5, dtype=torch.float32, device=be.dev),
        "emb": torch.zeros(V + 1, C, dtype=torch.bfloat16, device=be.dev),
        "x_out": nan_rows(be, B + 1, C),
        "token": torch.full((B + 2,), SENT, dtype=torch.int32, device=be.dev),
        "logit_prob": nan_rows(be, B + 1, 2, torch.float32),
    }
    return B, V, C, t


REJECTS = [
    # id                     sizes (B, V, C)      NULL              moved off its alignment     code
    ("B0",                   (0, 64, 16),         (),               (),                         EINVAL),
    ("B-1",                  (-1, 64, 16),        (),               (),                         EINVAL),
    ("V0",                   (2, 0, 16),          (),               (),                         ESHAPE),
    ("V12",                  (2, 12, 16),         (),               (),                         ESHAPE),
    ("Vcap+8",               (2, MAX_V + 8, 16),  (),               (),                         ESHAPE),
    ("C0",                   (2, 64, 0),          (),               (),                         ESHAPE),
    ("C12",                  (2, 64, 12),         (),               (),                         ESHAPE),
    ("null:logits",          (2, 64, 16),         ("logits",),      (),                         EINVAL),
    ("null:params",          (2, 64, 16),         ("params",),      (),                         EINVAL),
    ("null:u",               (2, 64, 16),         ("u",),           (),                         EINVAL),
    ("null:token",           (2, 64, 16),         ("token",),       (),                         EINVAL),
    ("null:logit_prob",      (2, 64, 16),         ("logit_prob",),  (),                         EINVAL),
    ("emb without x_out",    (2, 64, 16),         ("x_out",),       (),                         EINVAL),
    ("x_out without emb",    (2, 64, 16),         ("emb",),         (),                         EINVAL),
    ("off:logits",           (2, 64, 16),         (),               ("logits",),                EALIGN),
    ("off:emb",              (2, 64, 16),         (),               ("emb",),                   EALIGN),
    ("off:x_out",            (2, 64, 16),         (),               ("x_out",),                 EALIGN),
    ("off:params",           (2, 64, 16),         (),               ("params",),                EALIGN),
    ("off:u",                (2, 64, 16),         (),               ("u",),                     EALIGN),
    ("off:token",            (2, 64, 16),         (),               ("token",),                 EALIGN),
    ("off:logit_prob",       (2, 64, 16),         (),               ("logit_prob",),            EALIGN),
    # two faults: the count first, then the shape, then NULL, then the alignment
    ("B0 + V12",             (0, 12, 16),         (),               (),                         EINVAL),
    ("V12 + null:logits",    (2, 12, 16),         ("logits",),      (),                         ESHAPE),
    ("C12 + off:emb",        (2, 64, 12),         (),               ("emb",),                   ESHAPE),
    ("null:u + off:logits",  (2, 64, 16),         ("u",),           ("logits",),                EINVAL),
]


@pytest.mark.parametrize("backend,case", _params([r[0] for r in REJECTS]))
def test_rejects(backend, be, case):
    """The exact code, in the order count, shape, NULL, alignment; a refused call writes nothing."""
    _, sizes, nulls, offs, code = next(r for r in REJECTS if r[0] == case)
    _, _, _, t = _reject_setup(be)
    ptr = {}
    for name, buf in t.items():
        # off its alignment: 2 bytes (one bf16 element off a 16-byte piece; half a word for the scalars)
        ptr[name] = None if name in nulls else VP(buf.data_ptr() + 2) if name in offs else P(buf)
    before = {name: buf.clone() for name, buf in t.items()}
    rc = be.rc("vrwkv_sample_pick_bf16", ARGT, *sizes, *(ptr[n] for n in ("logits", "params", "u", "emb", "x_out", "token", "logit_prob")))
    if be.name == "hip":
        torch.cuda.synchronize()
    assert rc == code, (case, rc)
    for name, buf in t.items():
        assert torch.equal(bits(buf), bits(before[name])), f"{name} written"


@pytest.mark.parametrize("backend", BACKENDS)
def test_accepts_the_valid_call(backend, be):
    """The setup the rejections start from is itself accepted (with and without the embedding), and 4-byte aligned scalars are enough."""
    B, V, C, t = _reject_setup(be)
    args = lambda **kw: [kw.get(n, P(t[n])) for n in ("logits", "params", "u", "emb", "x_out", "token", "logit_prob")]      # noqa: E731
    assert be.rc("vrwkv_sample_pick_bf16", ARGT, B, V, C, *args()) == 0
    assert be.rc("vrwkv_sample_pick_bf16", ARGT, B, V, C, *args(emb=None, x_out=None)) == 0
    assert be.rc("vrwkv_sample_pick_bf16", ARGT, B, V, C, *args(u=VP(t["u"].data_ptr() + 4), token=VP(t["token"].data_ptr() + 4),
                                                                 params=VP(t["params"].data_ptr() + 8))) == 0
    if be.name == "hip":
        torch.cuda.synchronize()
    assert int(t["token"][-1]) == SENT and bool(torch.isnan(t["x_out"][B:].float()).all())
