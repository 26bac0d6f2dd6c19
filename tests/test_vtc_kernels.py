"""The two kernel families of the visual token compressor -- vrwkv_flip_add_bf16 (csrc/fused_ops.hip) and vrwkv_ln_pool_scatter_fwd_bf16 /
vrwkv_ln_pool_gather_bwd_bf16 (csrc/ln_fused.hip with csrc/ln_kernels.h: ln_out + unpad + AdaptiveAvgPool1d over tokens + scatter) -- through the
C ABI on the two backends of tests/test_ln_shapes.py: the host lockstep emulator (tests/emu/emu_fused_ops.cpp and emu_ln_fused.cpp compile the two
files whole) and the product library on an MI355X (`gpu` marker), with the same test bodies.  Helpers and bounds are those of test_glue_shapes.py,
test_ln_shapes.py and shape_checks.py, imported by name.

flip_add: out[b, T-1-t] = bf16(x[b, t] + delta[b, t]).  Bit-equal to the fp32 add rounded once and reversed, with and without delta, guard row
untouched, a second application (delta = NULL) gives the first one's input back, overlapping buffers are refused and nothing is written.
  (B, T, C)        what it reaches
  (1, 1, 64)       one token
  (2, 16, 64)      two samples
  (3, 17, 64)      odd T: the middle row maps to itself
  (1, 16, 8)       the narrowest C
  (2, 16, 8192)    the widest C
  (3, 4115, 64)    12 345 rows
  (3, 4115, 512)   790 080 16-byte pieces: more than the 2048 x 256 threads of the capped grid (asserted), the grid-stride loop's second trip

The tail, shapes (B, T, pad, Lout, C) with Lin = T - pad:
  identity  (2, 16, 0, 16, 64)     every window is one row
  ragged    (2, 32, 3, 4, 64)      29 -> 4: windows of 8 that overlap
  whole     (3, 32, 3, 1, 128)     one window per sample
  near      (1, 32, 15, 16, 64)    17 -> 16: every inner row in two windows
  real      (1, 736, 7, 64, 64)    729 -> 64: windows of 12-13
  w192 .. w8192  (1, 32, 3, 4, C)  C = 192, 2048, 2112, 4096, 8192: the block sizes of test_ln_shapes.py (a partial wave, 256 / 264 / 512 / 1024 threads)
  caps      (3, 1504, 4, 500, 64)  4512 rows over the backward's 1024 partial rows, 1500 outputs over the forward's 1024 workgroups
each dense (row_index = NULL) and scattered into a larger NaN-prefilled tensor through a permuted int64 row_index with three entries negative, each
with and without delta.  The pad rows of x and delta hold NaN: nothing of them may reach a result.

Reference: fp64 autograd on the CPU of LayerNorm (test_ln_shapes.ref_ln) -> unpad -> F.adaptive_avg_pool1d -> index, on the same bf16 inputs; it
rounds what the kernels round: xn = bf16(x + delta) where delta is given (test_ln_shapes.ste), and the final out / dx (Checks.act rounds once).
Bounds: test_ln_shapes.py's FLIP (out, xn, dx: Checks.act) and PERR (dw, db, mean, rstd: Checks.par and the statistics' figures of that module).
Also asserted: identity without delta gives out, mean and rstd of vrwkv_ln_scatter_fwd_bf16 bit for bit (and dx, dwb of vrwkv_ln_gather_bwd_bf16);
db is the fp64 column sum of the undropped dout rows; dx is exactly 0 on the pad rows; rows of `out` that no index names keep their bits; dropped
outputs leave the other rows of out as the dense call writes them, and the backward gives the bits of the same call with the dropped outputs pointed
at zero rows of dout; NaN-prefilled outputs and ws come back finite (but for the unspecified pad entries of xn, mean, rstd), the floats after
vrwkv_add_ln_ws_floats(B T, C) and every guard row stay NaN; a second call gives identical bits; bad arguments return the header's codes and write
nothing.
The emulator takes about 1 ms per row and kernel: `caps` (4512 rows, some 5 s per kernel) runs there once per form -- dense without delta, scattered with
delta -- and without the second call; the MI355X runs every case in full.
Observed worst over the module (VRWKV_TEST_NOTES=1 prints every figure):
  emulator: flips 4.883e-04 (real dense+delta out: two elements of 4096), parameter gradients and statistics 1.075e-06 (w8192 scatter dw)  --  bounds 1.2e-3, 3.3e-6
  MI355X:   flips 2.441e-04 (real dense out: one element of 4096), parameter gradients and statistics 8.999e-07 (w8192 dense dw)  --  bounds 3.7e-3, 3.8e-6
"""
import pytest
import torch
import torch.nn.functional as F

from tests.shape_checks import Checks
from tests.test_glue_shapes import F32, I, L, P, VP, bits, f64, nan_rows, rnd, same_bits, written
from tests.test_ln_shapes import EPS, FLIP, LN_BWD_GRID, PERR, TOL, LnBackend, nan_ws, ref_ln, ste

EINVAL, ESHAPE, EALIGN = -1, -2, -3
BACKENDS = ["emu", pytest.param("hip", marks=pytest.mark.gpu)]
FLIP_GRID_THREADS = 2048 * 256                 # fused_ops.hip: grid_for's cap x the workgroup size

CHECKS = Checks("vtc", FLIP, PERR, TOL)
note, act, par = CHECKS.note, CHECKS.act, CHECKS.par


@pytest.fixture
def be(request, backend):
    return LnBackend(request, backend)


def _params(rows):
    out = []
    for b in BACKENDS:
        name, marks = (b, ()) if isinstance(b, str) else (b.values[0], b.marks)
        for r in rows:
            if name == "emu" and r[0] == "caps" and r[1:] not in (("dense", "plain"), ("scatter", "delta")):
                continue
            out.append(pytest.param(name, *r, id="-".join((name,) + tuple(str(v) for v in r)), marks=marks))
    return out


# ------------------------------------------------------------------------------------------------ flip_add
FLIP_SHAPES = [(1, 1, 64), (2, 16, 64), (3, 17, 64), (1, 16, 8), (2, 16, 8192), (3, 4115, 64), (3, 4115, 512)]
FLIP_T = [I] * 3 + [VP] * 3


@pytest.mark.parametrize("backend,shape,cfg", _params([("x".join(map(str, s)), c) for s in FLIP_SHAPES for c in ("flip", "delta")]))
def test_flip_add(backend, be, shape, cfg):
    B, T, C = map(int, shape.split("x"))
    ntok = B * T
    if (B, T, C) == FLIP_SHAPES[-1]:
        assert ntok * C // 8 > FLIP_GRID_THREADS
    g = be.gen(31 * ntok + C + len(cfg))
    x = rnd(be, g, ntok, C)
    delta = rnd(be, g, ntok, C, scale=0.5) if cfg == "delta" else None
    want = x if delta is None else (x.float() + delta.float()).bfloat16()

    def run(src, d):
        out = nan_rows(be, ntok, C)
        be.call("vrwkv_flip_add_bf16", FLIP_T, B, T, C, P(src), P(d), P(out))
        assert bool(torch.isnan(out[-1].float()).all()), "guard row written"
        return out

    out = run(x, delta)
    assert torch.equal(bits(out[:-1]), bits(want.view(B, T, C).flip(1).reshape(ntok, C))), "not the rounded sum, reversed"
    assert torch.equal(bits(run(x, delta)), bits(out)), "the second call differs"
    back = run(out[:-1], None)                  # its own inverse (and its own backward)
    assert torch.equal(bits(back[:-1]), bits(want)), "two flips do not give the input back"


@pytest.mark.parametrize("backend", BACKENDS)
def test_flip_add_arguments(backend, be):
    B, T, C = 2, 4, 64
    g = be.gen(5)
    x, d = rnd(be, g, B * T + 1, C), rnd(be, g, B * T + 1, C)
    x0, d0 = x.clone(), d.clone()
    out = nan_rows(be, B * T, C)
    ok = [B, T, C, P(x), P(d), P(out)]

    def rc(**ch):
        a = list(ok)
        for k, v in ch.items():
            a[int(k[1:])] = v
        return be.rc("vrwkv_flip_add_bf16", FLIP_T, *a)

    assert rc(a5=P(x)) == EINVAL and rc(a5=P(d)) == EINVAL, "out aliases an input"
    assert rc(a5=P(x[1:])) == EINVAL and rc(a3=P(out[1:]), a4=None) == EINVAL, "out overlaps an input"
    assert rc(a0=0) == EINVAL and rc(a1=0) == EINVAL and rc(a3=None) == EINVAL and rc(a5=None) == EINVAL
    assert rc(a2=60) == ESHAPE and rc(a2=0) == ESHAPE
    for k, t in (("a3", x), ("a4", d), ("a5", out)):
        assert rc(**{k: VP(t.data_ptr() + 8)}) == EALIGN, (k, "8 bytes off a 16-byte boundary")
    assert rc(a5=VP(x.data_ptr() + 8)) == EINVAL and rc(a3=VP(out.data_ptr() + 8), a4=None) == EINVAL, "the overlap is found before the alignment"
    assert rc(a2=60, a3=VP(x.data_ptr() + 8)) == ESHAPE and rc(a3=None, a5=VP(out.data_ptr() + 8)) == EINVAL
    assert torch.equal(bits(x), bits(x0)) and torch.equal(bits(d), bits(d0)) and bool(torch.isnan(out.float()).all()), "a refused call wrote"
    assert rc() == 0 and rc(a4=None) == 0


# ------------------------------------------------------------------------------------------------ the tail
TAIL = {
    "identity": (2, 16, 0, 16, 64),
    "ragged": (2, 32, 3, 4, 64),
    "whole": (3, 32, 3, 1, 128),
    "near": (1, 32, 15, 16, 64),
    "real": (1, 736, 7, 64, 64),
    "w192": (1, 32, 3, 4, 192),
    "w2048": (1, 32, 3, 4, 2048),
    "w2112": (1, 32, 3, 4, 2112),
    "w4096": (1, 32, 3, 4, 4096),
    "w8192": (1, 32, 3, 4, 8192),
    "caps": (3, 1504, 4, 500, 64),
}
POOL_FWD_T = [I] * 5 + [F32] + [VP] * 9
POOL_BWD_T = [I] * 5 + [VP] * 9
EXTRA = 7                                       # rows of the scattered `out` that no index names


def pool_fwd(be, shp, x, delta, w, b, idx, nrows):
    B, T, pad, Lout, C = shp
    res = {"out": nan_rows(be, nrows, C), "mean": nan_rows(be, B * T, 1, torch.float32), "rstd": nan_rows(be, B * T, 1, torch.float32)}
    if delta is not None:
        res["xn"] = nan_rows(be, B * T, C)
    be.call("vrwkv_ln_pool_scatter_fwd_bf16", POOL_FWD_T, B, T, pad, Lout, C, EPS, P(x), P(delta), P(w), P(b), P(idx), P(res.get("xn")), P(res["out"]),
            P(res["mean"]), P(res["rstd"]))
    return res


def pool_bwd(be, shp, dout, idx, xn, f, w):
    B, T, pad, Lout, C = shp
    res = {"dx": nan_rows(be, B * T, C), "dwb": nan_rows(be, 2, C, torch.float32)}
    used = be.ws("vrwkv_add_ln_ws_floats", B * T, C)
    assert used == min(B * T, LN_BWD_GRID) * 2 * C
    ws = nan_ws(be, used, C)
    be.call("vrwkv_ln_pool_gather_bwd_bf16", POOL_BWD_T, B, T, pad, Lout, C, P(dout), P(idx), P(xn), P(f["mean"]), P(f["rstd"]), P(w), P(res["dx"]),
            P(res["dwb"]), P(ws))
    written(res, ws, used)
    return res


def ref_tail(shp, x, delta, w, b, real):
    """fp64, CPU: LayerNorm -> unpad -> adaptive_avg_pool1d.  Returns the leaf x, w, b, xn, the statistics and the (B Lout, C) pooled rows."""
    B, T, pad, Lout, C = shp
    keep = real.cpu()[:, None]
    xd, wd, bd = f64([torch.where(keep, x.cpu(), torch.zeros((), dtype=x.dtype)), w.cpu(), b.cpu()])
    xn = xd
    if delta is not None:
        xn = ste(xd + torch.where(keep, delta.cpu(), torch.zeros((), dtype=x.dtype)).double())
    y, st = ref_ln(xn, wd, bd)
    pooled = F.adaptive_avg_pool1d(y.view(B, T, C)[:, pad:].permute(0, 2, 1), Lout).permute(0, 2, 1).reshape(B * Lout, C)
    return xd, wd, bd, xn, st, pooled


def test_window_rule():
    """The kernels' windows, floor(i Lin / Lout) .. ceil((i + 1) Lin / Lout), are F.adaptive_avg_pool1d's; with Lout <= Lin a row lies in one or two."""
    for Lin, Lout in ((29, 4), (17, 16), (729, 64), (1458, 128), (29, 1), (16, 16), (1500, 500)):
        m = torch.zeros(Lout, Lin, dtype=torch.float64)
        for i in range(Lout):
            s, e = i * Lin // Lout, -(-(i + 1) * Lin // Lout)
            m[i, s:e] = 1.0 / (e - s)
        eye = torch.eye(Lin, dtype=torch.float64)
        assert torch.equal(F.adaptive_avg_pool1d(eye[None], Lout)[0].T, m), (Lin, Lout)
        cnt = (m > 0).sum(0)
        assert int(cnt.min()) >= 1 and int(cnt.max()) <= 2
        for t in range(Lin):                    # the backward's inverse rule
            i0, i1 = t * Lout // Lin, -(-(t + 1) * Lout // Lin) - 1
            assert torch.nonzero(m[:, t])[:, 0].tolist() == list(range(i0, i1 + 1)), (Lin, Lout, t)


@pytest.mark.parametrize("backend,sid,form,cfg", _params([(s, f, c) for s in TAIL for f in ("dense", "scatter") for c in ("plain", "delta")]))
def test_ln_pool(backend, be, sid, form, cfg):
    shp = B, T, pad, Lout, C = TAIL[sid]
    ntok, nout = B * T, B * Lout
    trimmed = be.name == "emu" and sid == "caps"
    g = be.gen(41 * ntok + C + Lout + len(form) + len(cfg))
    x, w, b = rnd(be, g, ntok, C), rnd(be, g, C, scale=0.5, shift=1.0), rnd(be, g, C, scale=0.3)
    delta = rnd(be, g, ntok, C, scale=0.5) if cfg == "delta" else None
    real = (torch.arange(ntok, device=be.dev) % T) >= pad
    x[~real] = float("nan")                     # the pad rows: never read
    if delta is not None:
        delta[~real] = float("nan")
    nrows = nout + (EXTRA if form == "scatter" else 0)
    dout = rnd(be, g, nrows, C)
    idx, keep = None, torch.ones(nout, dtype=torch.bool, device=be.dev)
    if form == "scatter":
        idx = torch.randperm(nrows, generator=torch.Generator().manual_seed(nout))[:nout].to(torch.int64)
        for k, o in enumerate(sorted({0, nout // 3, nout - 1}) if nout >= 6 else [nout // 2]):      # `whole`: 3 outputs, one dropped
            idx[o] = -1 - k
        idx = idx.to(be.dev)
        keep = idx >= 0
    rows = idx[keep] if idx is not None else torch.arange(nout, device=be.dev)
    tag = f"ln_pool/{sid}/{form}/{cfg}"

    def run(ix, d):
        f = pool_fwd(be, shp, x, delta, w, b, ix, nrows)
        for k in ("xn", "mean", "rstd"):
            if k in f:
                assert bool(torch.isfinite(f[k][:-1][real].float()).all()), f"{tag} {k}: not finite"
                assert bool(torch.isnan(f[k][-1].float()).all()), f"{tag} {k}: guard row written"
        assert bool(torch.isnan(f["out"][-1].float()).all()), f"{tag} out: guard row written"
        r = pool_bwd(be, shp, d, ix, f["xn"] if delta is not None else x, f, w)
        return {**f, **r}

    r1 = run(idx, dout)
    if not trimmed:
        r2 = run(idx, dout)
        for k in ("xn", "mean", "rstd"):        # the unspecified pad entries stay what they were: NaN in both
            if k in r1:
                r1[k][:-1][~real], r2[k][:-1][~real] = 0, 0
        same_bits(r1, r2)

    # rows of out: the named ones finite, the others untouched
    named = torch.zeros(nrows + 1, dtype=torch.bool, device=be.dev)
    named[rows] = True
    assert bool(torch.isfinite(r1["out"][named].float()).all()), f"{tag} out: not finite"
    assert bool(torch.isnan(r1["out"][~named].float()).all()), f"{tag}: a row that no index names was written"

    xd, wd, bd, xn, st, pooled = ref_tail(shp, x, delta, w, b, real)
    kc = keep.cpu()
    pooled[kc].backward(dout[rows].cpu().double())
    act(be, r1["out"][rows].cpu(), pooled[kc], f"{tag} out", guard=False)      # the reference lives on the CPU
    if delta is not None:
        act(be, r1["xn"][:-1][real].cpu(), xn[real.cpu()], f"{tag} xn", guard=False)
    m, r = r1["mean"][:-1, 0][real].double().cpu(), r1["rstd"][:-1, 0][real].double().cpu()
    rc_ = real.cpu()
    em = ((m - st["mean"][rc_]).abs() / (st["mean"][rc_].pow(2) + st["var"][rc_] + EPS).sqrt()).max()
    er = ((r - st["rstd"][rc_]).abs() / st["rstd"][rc_]).max()
    for kind, e in (("mean", float(em)), ("rstd", float(er))):
        note(be, "perr", e, f"{tag} {kind}")
        assert e < PERR[be.name], f"{tag} {kind}: worst row off by {e:.3e} (relative)"
    act(be, r1["dx"].cpu(), xd.grad, f"{tag} dx")
    assert not bool(r1["dx"][:-1][~real].float().abs().any()) and not bool(torch.isnan(r1["dx"][:-1].float()).any()), f"{tag}: dx of a pad row is not 0"
    assert not bool(bits(r1["dx"][:-1][~real]).any()), f"{tag}: dx of a pad row is not +0"
    par(be, r1["dwb"][0], wd.grad, f"{tag} dw")
    par(be, r1["dwb"][1], bd.grad, f"{tag} db")
    par(be, r1["dwb"][1], dout[rows].double().sum(0), f"{tag} db against the column sum of dout")

    if sid == "identity" and delta is None:     # one row per window: the LayerNorm + scatter entries, bit for bit
        ix = idx if idx is not None else torch.arange(nout, device=be.dev)
        s = {"out": nan_rows(be, nrows, C), "mean": nan_rows(be, ntok, 1, torch.float32), "rstd": nan_rows(be, ntok, 1, torch.float32),
             "dx": nan_rows(be, ntok, C), "dwb": nan_rows(be, 2, C, torch.float32)}
        be.call("vrwkv_ln_scatter_fwd_bf16", [L, I, F32] + [VP] * 7, ntok, C, EPS, P(x), P(w), P(b), P(ix), P(s["out"]), P(s["mean"]), P(s["rstd"]))
        ws = nan_ws(be, be.ws("vrwkv_add_ln_ws_floats", ntok, C), C)
        be.call("vrwkv_ln_gather_bwd_bf16", [L, I] + [VP] * 9, ntok, C, P(dout), P(ix), P(x), P(s["mean"]), P(s["rstd"]), P(w), P(s["dx"]), P(s["dwb"]), P(ws))
        same_bits(s, r1)

    if form == "scatter" and not trimmed:
        # dropped outputs: the kept rows of out are the dense call's; the backward is that of the same call with the dropped outputs' dout rows zero
        dense = pool_fwd(be, shp, x, delta, w, b, None, nout)
        assert torch.equal(bits(r1["out"][rows]), bits(dense["out"][:-1][keep])), f"{tag}: a dropped output changed another row of out"
        free = torch.nonzero(~named[:-1])[:, 0]
        idx0, dout0 = idx.clone(), dout.clone()
        idx0[~keep] = free[:int((~keep).sum())]
        dout0[idx0[~keep]] = 0
        rz = pool_bwd(be, shp, dout0, idx0, r1["xn"] if delta is not None else x, r1, w)
        same_bits(rz, {k: r1[k] for k in rz})


@pytest.mark.parametrize("backend", BACKENDS)
def test_ln_pool_arguments(backend, be):
    """What the two entries refuse, by return code; nothing is launched, nothing written."""
    B, T, pad, Lout, C = 2, 16, 3, 4, 64
    t = torch.zeros(B * T + 1, C, dtype=torch.float32, device=be.dev)
    outs = [torch.full((B * T + 1, C), float("nan"), dtype=torch.float32, device=be.dev) for _ in range(5)]
    p = P(t)
    o = [P(v) for v in outs]
    fwd = [B, T, pad, Lout, C, EPS, p, p, p, p, None, o[0], o[1], o[2], o[3]]
    bwd = [B, T, pad, Lout, C, p, None, p, p, p, p, o[0], o[1], o[4]]

    def rc(which, **ch):
        a = list(fwd if which == "fwd" else bwd)
        for k, v in ch.items():
            a[int(k[1:])] = v
        return be.rc("vrwkv_ln_pool_scatter_fwd_bf16" if which == "fwd" else "vrwkv_ln_pool_gather_bwd_bf16", POOL_FWD_T if which == "fwd" else POOL_BWD_T, *a)

    for which, required in (("fwd", (6, 8, 9, 12, 13, 14)), ("bwd", (5, 7, 8, 9, 10, 11, 12, 13))):
        assert rc(which, a3=T - pad + 1) == ESHAPE, (which, "Lout > Lin")
        assert rc(which, a3=0) == ESHAPE and rc(which, a3=-1) == ESHAPE, (which, "Lout < 1")
        for c in (96, 8, 8256):
            assert rc(which, a4=c) == ESHAPE, (which, "C", c)
        assert rc(which, a0=0) == EINVAL and rc(which, a1=0) == EINVAL and rc(which, a2=-1) == EINVAL and rc(which, a2=T) == EINVAL, (which, "sizes")
        for k in required:
            assert rc(which, **{f"a{k}": None}) == EINVAL, (which, "NULL argument", k)
    assert rc("fwd", a11=None) == EINVAL, "delta without xn"
    assert all(bool(torch.isnan(v).all()) for v in outs), "a refused call wrote"
    assert rc("fwd", a7=None, a11=None) == 0
