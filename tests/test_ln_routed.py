"""The modality-routed channel-mix entries of csrc/ln_fused.hip -- vrwkv_ln_mix_routed_fwd_bf16, vrwkv_ln_mix_routed_bwd_bf16 (the ROUTED
instantiations of ln_mix_fwd_kernel / ln_mix_bwd_kernel, M = 1) and vrwkv_row_gather_bf16 -- through the C ABI on the two backends of
tests/test_ln_shapes.py: the host lockstep emulator (tests/emu/emu_ln_fused.cpp compiles ln_fused.hip whole) and the product library on
an MI355X (`gpu` marker).  Helpers, reference pieces and the two bounds are those of test_ln_shapes.py.

What is routed.  Row n goes through expert e(n) = sel[n] != 0: LayerNorm (w_e, b_e) and lerp weight mu_e; its shifted value is the row before
under ROW n's expert, LN_e(n)(xn[n-1]); the statistics of a row are shared.  out is written at pos[n], dout read there.  The backward keeps
the parameters and partial sums of one expert in registers and changes them where e(n) != e(n-1) (ln_kernels.h: ln_mix_bwd_routed), so the
masks place expert changes at a workgroup's first row, inside a range, at its look-ahead row hi, on every row, and never.

  shape      (B, T, C)        what it reaches
  one        (1, 1, 256)      one token
  b2         (2, 16, 1024)    two samples, eight forward ranges
  b3         (3, 48, 2048)    256 threads full: the <256> backward
  wide       (2, 16, 4096)    the largest C the entries serve: the <512> backward
  cap        (3, 800, 64)     2400 rows over the backward's 768 workgroups: ranges of 3-4 rows with the look-ahead row
  masks: text | image | alt (every shift crosses experts) | range (changes exactly at the backward's range starts: all rows of a range
  one expert, the look-ahead row the other) | block (an image block in the middle of every sample) | tok0 (an image token at n % T == 0);
  each plain (first = NULL, int32 pos) and packed (drawn first marks, int64 pos).

Asserted, as the points (a) .. (e) of the docstrings below:
  (a) forward: out[pos[n]] is bit for bit row n of vrwkv_ln_mix_fwd_packed_bf16 run on the whole input with expert e(n)'s parameters;
      xn, mean, rstd are that entry's.
  (b) a uniform mask with identity pos: forward and backward (dx, the live expert's dwb and dmu) are the plain entries bit for bit, the
      dead expert's gradients exactly 0.
  (c) mixed masks: dx, dwb[2], dmu[2] against fp64 autograd of the `where` statement on the same bf16 inputs, under test_ln_shapes.py's
      FLIP and PERR by value.  The reference rounds what the kernels round: xn, each expert's LayerNorm output, and the gradient that
      arrives at each expert's LayerNorm output (test_ln_shapes.RoundGrad; where both terms of a row come through one expert they are
      summed before the rounding, as in the plain kernel).
  (d) NaN-prefilled outputs come back finite, guard rows and the floats after ws untouched, a second call bit-identical.
  (e) the gather and its inverse are exact.
On the emulator the `cap` shape (14 s per case) runs the masks alt and range, and image once for (b); the MI355X runs every case.
The emulator walks the rows of C >= 2048 (about 1 ms per row and kernel) with fewer tokens, as test_ln_shapes.py does: `b3` as (3, 16, 2048), `wide`
as (2, 8, 4096); the (3, 48) and (2, 16) forms of those two shapes run on the MI355X only.  (B, T) = (2, 16) is reached on both at C = 1024.
Observed worst over the module (VRWKV_TEST_NOTES=1 prints every figure; all masks of `cap` included):
  emulator: flips 7.161e-05 (cap alt plain dx), parameter gradients 1.001e-06 (wide range packed dw1)  --  bounds 1.2e-3, 3.3e-6
  MI355X:   flips 6.104e-05 (b2 range packed dx), parameter gradients 8.742e-07 (wide block packed dmu1)  --  bounds 3.7e-3, 3.8e-6
"""
import pytest
import torch

from tests.shape_checks import Checks
from tests.test_glue_shapes import F32, I, L, P, PA, VP, bits, f64, nan_rows, rnd, same_bits, unif, written
from tests.test_ln_shapes import (EPS, LN_MIX_BWD_GRID, LnBackend, RoundGrad, add_ln_fwd, nan_ws, near_tie, ranges, ref_ln, ste)

TOL = 1e-3
FLIP = {"emu": 1.2e-3, "hip": 3.7e-3}          # test_ln_shapes.py's bounds for ln_mix M = 1, by value
PERR = {"emu": 3.3e-6, "hip": 3.8e-6}
EINVAL, ESHAPE = -1, -2

BACKENDS = ["emu", pytest.param("hip", marks=pytest.mark.gpu)]
SHAPES = {"one": (1, 1, 256), "b2": (2, 16, 1024), "b3": (3, 48, 2048), "wide": (2, 16, 4096), "cap": (3, 800, 64)}
MASKS = ["text", "image", "alt", "range", "block", "tok0"]
UNIFORM = ("text", "image")
EMU_CAP_MASKS = ("alt", "range")

CHECKS = Checks("routed", FLIP, PERR, TOL)
note, act, par = CHECKS.note, CHECKS.act, CHECKS.par

FWD_T = [L, I, I, F32] + [VP] * 12 + [I]
BWD_T = [L, I, I] + [VP] * 11 + [I] + [VP] * 4
PACKED_FWD_T = [L, I, I, F32, I] + [VP] * 10
PACKED_BWD_T = [L, I, I, I] + [VP] * 14


@pytest.fixture
def be(request, backend):
    return LnBackend(request, backend)


def _cases(masks=MASKS, shapes=SHAPES):
    out = []
    for b in BACKENDS:
        name, marks = (b, ()) if isinstance(b, str) else (b.values[0], b.marks)
        for sid in shapes:
            for mask in masks:
                for form in ("plain", "packed"):
                    if sid == "one" and (form == "packed" or mask not in ("text", "image")):
                        continue
                    if name == "emu" and sid == "cap" and not (mask in EMU_CAP_MASKS or (mask == "image" and form == "plain")):
                        continue                       # 2400 rows take the emulator 14 s per case
                    out.append(pytest.param(name, sid, mask, form, id=f"{name}-{sid}-{mask}-{form}", marks=marks))
    return out


def make_sel(sid, mask, B, T):
    ntok = B * T
    n = torch.arange(ntok)
    if mask == "text":
        sel = torch.zeros(ntok, dtype=torch.bool)
    elif mask == "image":
        sel = torch.ones(ntok, dtype=torch.bool)
    elif mask == "alt":
        sel = n % 2 == 1
    elif mask == "range":                      # every range of the backward one expert, its neighbours the other
        sel = torch.zeros(ntok, dtype=torch.bool)
        for g, (lo, hi) in enumerate(ranges(ntok, min(ntok, LN_MIX_BWD_GRID))):
            sel[lo:hi] = g % 2 == 1
        if ntok <= LN_MIX_BWD_GRID:            # one row per range: that is `alt`; change every third row instead
            sel = (n // 3) % 2 == 1
    elif mask == "block":
        sel = ((n % T) >= T // 4) & ((n % T) < T // 4 + max(1, T // 2))
    else:                                      # tok0: an image token at the first position of every sample, one more mid-row
        sel = (n % T == 0) | (n % T == T // 2)
    return sel.to(torch.uint8)


def make_first(ntok, T, sel):
    """Packed marks: at an expert change, one row after a change, inside a run, a one-token segment."""
    first = torch.zeros(ntok, dtype=torch.uint8)
    if ntok < 4:
        return first
    ch = torch.nonzero(sel[1:] != sel[:-1])[:, 0] + 1
    if len(ch):
        first[ch[len(ch) // 2]] = 1
        if ch[0] + 1 < ntok:
            first[ch[0] + 1] = 1
    first[ntok // 2] = 1
    first[ntok // 2 + 1] = 1
    first[torch.randint(1, ntok, (max(1, ntok // 40),), generator=torch.Generator().manual_seed(ntok))] = 1
    return first


def make_pos(sel, identity):
    """Image rows first, then text rows, each group in token order (fused.RoutePlan); pos[n] = the routed row of token n."""
    ntok = sel.numel()
    if identity:
        return torch.arange(ntok)
    order = torch.argsort(sel == 0, stable=True)
    pos = torch.empty(ntok, dtype=torch.long)
    pos[order] = torch.arange(ntok)
    return pos


class Case:
    def __init__(self, be, sid, mask, form, identity=False):
        B, T, C = SHAPES[sid]
        if be.name == "emu" and C >= 2048:
            T = 16 if sid == "b3" else 8                    # about 1 ms per row and kernel on the emulator
        self.B, self.T, self.C, self.ntok = B, T, C, B * T
        ntok = B * T
        g = be.gen(31 * ntok + C + sum(map(ord, mask + form)))
        self.x, self.delta = rnd(be, g, ntok, C), rnd(be, g, ntok, C, scale=0.5)
        self.w = [rnd(be, g, C, scale=0.5, shift=1.0) for _ in range(2)]
        self.b = [rnd(be, g, C, scale=0.3) for _ in range(2)]
        self.mu = [unif(be, g, C) for _ in range(2)]
        self.dout, self.dres = rnd(be, g, ntok, C), rnd(be, g, ntok, C)
        sel = make_sel(sid, mask, B, T)
        self.sel = sel.to(be.dev)
        self.first = make_first(ntok, T, sel).to(be.dev) if form == "packed" else None
        pos = make_pos(sel, identity)
        self.pos64 = form == "packed"
        self.pos_l = pos.to(be.dev)
        self.pos = (pos if self.pos64 else pos.to(torch.int32)).to(be.dev)
        self.tag = f"routed/{sid}/{mask}/{form}"


def routed_fwd(be, c):
    res = {"out": nan_rows(be, c.ntok, c.C), "xn": nan_rows(be, c.ntok, c.C), "mean": nan_rows(be, c.ntok, 1, torch.float32),
           "rstd": nan_rows(be, c.ntok, 1, torch.float32)}
    be.call("vrwkv_ln_mix_routed_fwd_bf16", FWD_T, c.ntok, c.T, c.C, EPS, P(c.x), P(c.delta), PA(c.w), PA(c.b), PA(c.mu), P(res["xn"]), P(res["out"]),
            P(res["mean"]), P(res["rstd"]), P(c.first), P(c.sel), P(c.pos), 8 if c.pos64 else 4)
    written(res, None, 0)
    return res


def routed_bwd(be, c, f):
    res = {"dx": nan_rows(be, c.ntok, c.C), "dwb": nan_rows(be, 4, c.C, torch.float32), "dmu": nan_rows(be, 2, c.C, torch.float32)}
    used = be.ws("vrwkv_ln_mix_routed_ws_floats", c.ntok, c.C)
    assert used == min(c.ntok, LN_MIX_BWD_GRID) * 6 * c.C
    ws = nan_ws(be, used, c.C)
    be.call("vrwkv_ln_mix_routed_bwd_bf16", BWD_T, c.ntok, c.T, c.C, P(f["xn"]), P(f["mean"]), P(f["rstd"]), PA(c.w), PA(c.b), PA(c.mu), P(c.dout), P(c.dres),
            P(c.first), P(c.sel), P(c.pos), 8 if c.pos64 else 4, P(res["dx"]), P(res["dwb"]), P(res["dmu"]), P(ws))
    written(res, ws, used)
    return res


def plain_fwd(be, c, e):
    res = {"out": nan_rows(be, c.ntok, c.C), "xn": nan_rows(be, c.ntok, c.C), "mean": nan_rows(be, c.ntok, 1, torch.float32),
           "rstd": nan_rows(be, c.ntok, 1, torch.float32)}
    be.call("vrwkv_ln_mix_fwd_packed_bf16", PACKED_FWD_T, c.ntok, c.T, c.C, EPS, 1, P(c.x), P(c.delta), P(c.w[e]), P(c.b[e]), PA([c.mu[e]]), P(res["xn"]),
            PA([res["out"]]), P(res["mean"]), P(res["rstd"]), P(c.first))
    return res


def plain_bwd(be, c, e, f):
    res = {"dx": nan_rows(be, c.ntok, c.C), "dwb": nan_rows(be, 2, c.C, torch.float32), "dmu": nan_rows(be, 1, c.C, torch.float32)}
    ws = nan_ws(be, be.ws("vrwkv_ln_mix_ws_floats", c.ntok, c.C, 1), c.C)
    be.call("vrwkv_ln_mix_bwd_packed_bf16", PACKED_BWD_T, c.ntok, c.T, c.C, 1, P(f["xn"]), P(f["mean"]), P(f["rstd"]), P(c.w[e]), P(c.b[e]), PA([c.mu[e]]),
            PA([c.dout]), None, P(c.dres), P(c.first), P(res["dx"]), P(res["dwb"]), P(res["dmu"]), P(ws))
    return res


# ------------------------------------------------------------------------------------------------ (a), (d): the forward
@pytest.mark.parametrize("backend,sid,mask,form", _cases())
def test_forward_rows_are_the_plain_kernel_with_the_rows_expert(backend, be, sid, mask, form):
    """(a) and the forward half of (d)."""
    c = Case(be, sid, mask, form)
    r1 = routed_fwd(be, c)
    same_bits(r1, routed_fwd(be, c))
    p = [plain_fwd(be, c, 0), plain_fwd(be, c, 1)]
    for k in ("xn", "mean", "rstd"):
        assert torch.equal(bits(r1[k]), bits(p[0][k])), f"{c.tag} {k}: differs from vrwkv_ln_mix_fwd_packed_bf16"
    want = torch.where(c.sel[:, None] != 0, p[1]["out"][:-1], p[0]["out"][:-1])
    got = r1["out"][:-1][c.pos_l]
    bad = torch.nonzero((bits(got) != bits(want)).any(dim=1))[:, 0]
    assert bad.numel() == 0, f"{c.tag}: out[pos[n]] differs from the plain kernel with expert sel[n] at rows {bad[:8].tolist()} of {c.ntok}"


# ------------------------------------------------------------------------------------------------ (b): uniform masks
@pytest.mark.parametrize("backend,sid,mask,form", _cases(UNIFORM))
def test_uniform_mask_is_the_plain_entry(backend, be, sid, mask, form):
    """(b): one expert on every row, identity pos."""
    c = Case(be, sid, mask, form, identity=True)
    e = int(mask == "image")
    f = routed_fwd(be, c)
    r = routed_bwd(be, c, f)
    pf = plain_fwd(be, c, e)
    pb = plain_bwd(be, c, e, pf)
    same_bits({k: f[k] for k in ("out", "xn", "mean", "rstd")}, pf)
    assert torch.equal(bits(r["dx"]), bits(pb["dx"])), f"{c.tag}: dx"
    assert torch.equal(bits(r["dwb"][2 * e:2 * e + 2]), bits(pb["dwb"][:2])), f"{c.tag}: dwb of the live expert"
    assert torch.equal(bits(r["dmu"][e]), bits(pb["dmu"][0])), f"{c.tag}: dmu of the live expert"
    d = 1 - e
    assert not bool(r["dwb"][2 * d:2 * d + 2].any()) and not bool(r["dmu"][d].any()), f"{c.tag}: the dead expert has a gradient"


# ------------------------------------------------------------------------------------------------ (c), (d): mixed masks against fp64
def ref_routed(c, y_got):
    """fp64 autograd of x + where(sel, lerp_1(LN_1(xn)), lerp_0(LN_0(xn))) on the bf16 inputs, with the kernels' roundings (module docstring)."""
    xd, dd = c.x.double().requires_grad_(True), c.delta.double()
    wd, bd, md = f64(c.w), f64(c.b), f64(c.mu)
    xn = ste(xd + dd)
    n = torch.arange(c.ntok, device=c.x.device)
    opens = (n % c.T == 0)
    if c.first is not None:
        opens = opens | (c.first != 0)
    outs, st = [], None
    for e in range(2):
        yf, st = ref_ln(xn, wd[e], bd[e])
        yq = yf + (near_tie(yf.detach(), y_got[e]) - yf.detach())
        y = RoundGrad.apply(yq, None, {})
        sh = torch.cat([torch.zeros(1, c.C, dtype=torch.float64, device=c.x.device), y[:-1]])
        sh = torch.where(opens[:, None], torch.zeros_like(sh), sh)
        outs.append(y + (sh - y) * md[e])
    out = torch.where(c.sel[:, None] != 0, outs[1], outs[0])
    out.backward(c.dout[c.pos_l].double())
    return {"out": out, "dx": xd.grad + c.dres.double(), "dw": [w.grad for w in wd], "db": [b.grad for b in bd], "dmu": [m.grad for m in md], "st": st}


@pytest.mark.parametrize("backend,sid,mask,form", _cases([m for m in MASKS if m not in UNIFORM]))
def test_mixed_mask_against_fp64_autograd(backend, be, sid, mask, form):
    """(c) and the backward half of (d)."""
    c = Case(be, sid, mask, form)
    f = routed_fwd(be, c)
    r1 = routed_bwd(be, c, f)
    same_bits(r1, routed_bwd(be, c, f))
    y_got = [add_ln_fwd(be, c.ntok, c.C, c.x, c.delta, c.w[e], c.b[e])["y"][:-1] for e in range(2)]
    ref = ref_routed(c, y_got)
    act(be, f["out"][:-1][c.pos_l], ref["out"], f"{c.tag} out", guard=False)
    act(be, r1["dx"], ref["dx"], f"{c.tag} dx")
    for e in range(2):
        par(be, r1["dwb"][2 * e], ref["dw"][e], f"{c.tag} dw{e}")
        par(be, r1["dwb"][2 * e + 1], ref["db"][e], f"{c.tag} db{e}")
        par(be, r1["dmu"][e], ref["dmu"][e], f"{c.tag} dmu{e}")


# ------------------------------------------------------------------------------------------------ (e): the gather
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("n,C,idx_bytes", [(1, 64, 4), (37, 200, 8), (1125, 2048, 4)])
def test_row_gather_and_its_inverse_are_exact(backend, be, n, C, idx_bytes):
    """(e): dst[i] = src[idx[i]]; gathering again with the inverse permutation gives src back; guard rows untouched."""
    g = be.gen(n + C)
    src = rnd(be, g, n, C)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(n))
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(n)
    dt = torch.int64 if idx_bytes == 8 else torch.int32
    idx, iidx = perm.to(dt).to(be.dev), inv.to(dt).to(be.dev)
    T_ = [L, I, VP, VP, I, VP]
    a, b2 = nan_rows(be, n, C), nan_rows(be, n, C)
    be.call("vrwkv_row_gather_bf16", T_, n, C, P(src), P(idx), idx_bytes, P(a))
    be.call("vrwkv_row_gather_bf16", T_, n, C, P(a), P(iidx), idx_bytes, P(b2))
    written({"a": a, "b": b2}, None, 0)
    assert torch.equal(bits(a[:-1]), bits(src[perm.to(be.dev)]))
    assert torch.equal(bits(b2[:-1]), bits(src))


# ------------------------------------------------------------------------------------------------ argument checks
@pytest.mark.parametrize("backend", BACKENDS)
def test_arguments(backend, be):
    """What the entries refuse, by return code; nothing is launched."""
    ntok, T, C = 8, 4, 64
    t = torch.zeros(64, 64, dtype=torch.float32, device=be.dev)
    p, arr = P(t), PA([t] * 2)
    fwd = [ntok, T, C, EPS, p, p, arr, arr, arr, p, p, p, p, p, p, p, 4]
    bwd = [ntok, T, C, p, p, p, arr, arr, arr, p, p, p, p, p, 4, p, p, p, p]

    def rc(fn, types, args, **change):
        args = list(args)
        for k, v in change.items():
            args[int(k[1:])] = v
        return be.rc(fn, types, *args)

    holed = (VP * 2)(t.data_ptr(), None)
    for fn, types, args, req, arrs, pb in (("vrwkv_ln_mix_routed_fwd_bf16", FWD_T, fwd, (4, 6, 7, 8, 10, 11, 12, 14, 15), (6, 7, 8), 16),
                                           ("vrwkv_ln_mix_routed_bwd_bf16", BWD_T, bwd, (3, 4, 5, 6, 7, 8, 9, 12, 13, 15, 16, 17, 18), (6, 7, 8), 14)):
        for cbad in (96, 4160, 8192):
            assert rc(fn, types, args, a2=cbad) == ESHAPE, (fn, cbad)
        assert rc(fn, types, args, a0=0) == EINVAL and rc(fn, types, args, a0=ntok + 1) == EINVAL
        for k in req:
            assert rc(fn, types, args, **{f"a{k}": None}) == EINVAL, (fn, k)
        for k in arrs:
            assert rc(fn, types, args, **{f"a{k}": holed}) == EINVAL, (fn, k)
        assert rc(fn, types, args, **{f"a{pb}": 2}) == EINVAL
    assert rc("vrwkv_ln_mix_routed_fwd_bf16", FWD_T, fwd, a9=None) == EINVAL            # delta without xn
    g = [4, 64, p, p, 4, p]
    GT = [L, I, VP, VP, I, VP]
    assert rc("vrwkv_row_gather_bf16", GT, g, a1=12) == ESHAPE and rc("vrwkv_row_gather_bf16", GT, g, a4=2) == EINVAL
    assert rc("vrwkv_row_gather_bf16", GT, g, a0=0) == EINVAL and rc("vrwkv_row_gather_bf16", GT, g, a3=None) == EINVAL
