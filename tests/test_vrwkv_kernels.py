"""The kernels of the trainable RWKV vision encoder (VisualRWKV-v7/v7.10 `vrwkv`) through the C ABI, on the two backends of
tests/test_wgrad_shapes.py and tests/test_vtc_kernels.py with the same test bodies: the host lockstep emulator (tests/emu/emu_lora_wgrad.cpp and
emu_ln_fused.cpp compile csrc/lora_wgrad.hip and csrc/ln_fused.hip whole, so the launch logic is the product's own) and the product library on
an MI355X (`gpu` marker).  Helpers and bounds are imported from those modules by name.
The emulator's vmem_wait is a no-op: the LDS-DMA waits and barriers of the weight-gradient kernel's ring are tested on the MI355X only.

vrwkv_patch_embed_wgrad_bf16 (csrc/patch_wgrad.h): dW (N x 768) = dout^T patches(pixels), dbias = column sums of dout.
  Oracle: dout.double().T @ F.unfold(pixels.double(), 16, stride=16) rearranged to (B Mimg, 768); test_conv2d_order pins the (c, py, px) order of
  that oracle against torch.autograd.grad of an fp64 F.conv2d.  The three oracles of test_wgrad_shapes.py's docstring:
    exact      integers in [-8, 8]: the result EQUALS the fp64 product rounded to bf16 at every element (B Mimg <= 262 144); dbias too
    float      randn x 0.5 pixels, randn x 0.3 dout: |out - exact| <= U (|exact| + E) + E with that module's derived U and E at this launch's M and
               slice count (dbias: M + 8 row lanes + its row slices terms), bf16_close(tol=1e-3, max_flip=0.02) and group_bias
    selection  real pixels, dout = 1.0 at one (row, channel): that row of dW holds the patch's pixel bits, every other row is zero
  (grid, B) -> rows, what it reaches (slices S = min(8, stages) at N = 256 and 512: 3 and 6 tiles):
    2 x 4, 4        32     one stage that holds four images, S = 1: the bf16 epilogue
    4 x 2, 4        32     gy / gx swapped
    3 x 5, 32       480    15 stages, S = 8: one and two stages per slice, Mimg = 15 and gw = 5 are not powers of two, images straddle every stage
    8 x 8, 1 .. 3   64 .. 192   2, 4, 6 stages = slices of one stage
    8 x 8, 12, 16, 24, 32      768 .. 2048 rows: 3, 4, 6, 8 stages per slice (the ring's steady state and every tail of test_big_stages)
  N = 256 and 512 (T1 = 1 and 2 against T2 = 3).  Every case: return code 0; dW and dbias inside NaN buffers with 32-element guards, ws NaN and
  followed by a guard, three NaN rows behind dout and a NaN image behind the last one; a second call is bit-identical; dbias NULL is accepted.
  Thinned on the emulator (it walks a stage of one tile in about 60 ms): the 8 x 8 cases with B >= 12 run N = 256 and the exact oracle only, once;
  the float oracle runs at 2 x 4, 3 x 5 and 8 x 8 with B = 2.  The MI355X runs everything.
  Refused with the exact code, -1 from the size function and untouched outputs: P = 14, N = 128, B Mimg = 48, Wimg = 24, a misaligned pointer.

vrwkv_ln_scatter_mean_fwd_bf16 / vrwkv_ln_gather_mean_bwd_bf16 (csrc/ln_kernels.h): ln_out over all rows scattered through row_index plus the mean
  over tokens for the ImageNet head.  Oracle: fp64 autograd of test_ln_shapes.ref_ln on the same bf16 inputs, rounding what the kernels round
  (xn = bf16(x + delta): ste); bounds Checks("vrwkv", FLIP, PERR, TOL) of test_ln_shapes.py.
  (B, L, C): (1,1,64) a single row; (2,16,64); (3,17,128) odd L; (1,16,8192) the widest row; (2,600,64) 1200 rows: the forward's 64 partial rows per
  sample with ranges of 9 and 10 rows, the backward's 1024 partial rows; (5,256,512) v7.10's tokens per image.
  row_index: NULL; a permutation into a tensor with 7 more rows (which keep their bits); every third entry -1; one whole sample -1 (its pooled row
  must still be right).  delta NULL and given.  Backward with both sources, dout only, dpooled only.
  Bit for bit: the scattered rows, xn, mean and rstd equal vrwkv_ln_pool_scatter_fwd_bf16 (Lout = L, pad = 0) and, without delta,
  vrwkv_ln_scatter_fwd_bf16; with dpooled NULL dx and dwb equal vrwkv_ln_gather_bwd_bf16.  pooled is checked against fp64 only (its summation
  order is its own).  NaN-prefilled outputs come back finite, guard rows and the floats behind vrwkv_ln_scatter_mean_ws_floats stay NaN, a second
  call gives the same bits, bad arguments return the header's codes and write nothing.
  Thinned on the emulator (about 1 ms per row and kernel, 0.1 s per row of 1024 threads): (1,16,8192), (2,600,64) and (5,256,512) run four of the
  eight (row_index, delta) pairs -- every row_index form once, delta alternating -- without the second call.  With everything the 61 emulator
  cases took 220 s; thinned, 57 cases take 186 s on a machine that ran another suite beside them (the slowest 12 s).  The 73 MI355X cases take 3.6 s.
"""
import pytest
import torch
import torch.nn.functional as F

from tests.parity import bf16_close, group_bias
from tests.shape_checks import Checks
from tests.test_glue_shapes import F32, I, L, P, VP, bits, f64, nan_rows, rnd, same_bits
from tests.test_ln_shapes import EPS, FLIP, LN_BWD_GRID, PERR, TOL, LnBackend, nan_ws, ref_ln, ste
from tests.test_wgrad_shapes import EALIGN, EINVAL, ESHAPE, GUARD, MAX_FLIP, NAN, U, big_splits
from tests.test_wgrad_shapes import TOL as WTOL

BACKENDS = ["emu", pytest.param("hip", marks=pytest.mark.gpu)]
CHECKS = Checks("vrwkv", FLIP, PERR, TOL)
note, act, par = CHECKS.note, CHECKS.act, CHECKS.par
K = 768


@pytest.fixture
def be(request, backend):
    return LnBackend(request, backend)


def _params(rows, skip_emu=lambda r: False):
    out = []
    for b in BACKENDS:
        name, marks = (b, ()) if isinstance(b, str) else (b.values[0], b.marks)
        for r in rows:
            r = r if isinstance(r, tuple) else (r,)
            if name == "emu" and skip_emu(r):
                continue
            out.append(pytest.param(name, *r, id="-".join((name,) + tuple(str(v) for v in r)), marks=marks))
    return out


# ------------------------------------------------------------------------------------------------ patch-embedding weight gradient
WG_T = [I] * 5 + [VP] * 5
WG_CASES = [(2, 4, 4), (4, 2, 4), (3, 5, 32), (8, 8, 1), (8, 8, 2), (8, 8, 3), (8, 8, 12), (8, 8, 16), (8, 8, 24), (8, 8, 32)]
EMU_FLOAT = ((2, 4, 4), (3, 5, 32), (8, 8, 2))


def wg_size(be, B, H, W, Pp, N):
    f = be.lib.vrwkv_patch_embed_wgrad_ws_floats
    f.argtypes, f.restype = [I] * 5, L
    return int(f(B, H, W, Pp, N))


def unfolded(pixels, gh, gw):
    """(B, 3, 16 gh, 16 gw) -> fp64 (B gh gw, 768), column (c 16 + py) 16 + px."""
    B = pixels.shape[0]
    return F.unfold(pixels.double().cpu(), 16, stride=16).permute(0, 2, 1).reshape(B * gh * gw, K)


def wg_inputs(be, g, kind, B, gh, gw, N):
    M = B * gh * gw
    px = torch.full((B + 1, 3, 16 * gh, 16 * gw), NAN, dtype=torch.bfloat16, device=be.dev)          # a NaN image behind the last one
    do = torch.full((M + 3, N), NAN, dtype=torch.bfloat16, device=be.dev)                            # three NaN rows behind dout
    if kind == "exact":
        px[:B] = torch.randint(-8, 9, px[:B].shape, generator=g, device=be.dev).bfloat16()
        do[:M] = torch.randint(-8, 9, (M, N), generator=g, device=be.dev).bfloat16()
    else:
        px[:B] = (torch.randn(px[:B].shape, generator=g, device=be.dev) * 0.5).bfloat16()
        do[:M] = (torch.randn(M, N, generator=g, device=be.dev) * 0.3).bfloat16()
    return px, do


def wg_call(be, B, gh, gw, N, px, do, ws_n, bias=True, tag=""):
    dw = torch.full((GUARD + N * K + GUARD,), NAN, dtype=torch.bfloat16, device=be.dev)
    db = torch.full((GUARD + N + GUARD,), NAN, dtype=torch.bfloat16, device=be.dev)
    ws = torch.full((ws_n + GUARD,), NAN, dtype=torch.float32, device=be.dev)
    rc = be.rc("vrwkv_patch_embed_wgrad_bf16", WG_T, B, 16 * gh, 16 * gw, 16, N, P(px), P(do), VP(dw.data_ptr() + 2 * GUARD),
               VP(db.data_ptr() + 2 * GUARD) if bias else None, P(ws))
    assert rc == 0, (tag, rc)
    for name, buf in (("dW", dw), ("dbias", db)):
        assert bool(torch.isnan(buf[:GUARD].float()).all()) and bool(torch.isnan(buf[-GUARD:].float()).all()), f"{tag}: a guard of {name} was written"
    assert bool(torch.isfinite(dw[GUARD:-GUARD].float()).all()), f"{tag}: dW is not finite (unwritten, or NaN rows / pixels / scratch were read)"
    if bias:
        assert bool(torch.isfinite(db[GUARD:-GUARD].float()).all()), f"{tag}: dbias is not finite"
    else:
        assert bool(torch.isnan(db.float()).all()), f"{tag}: dbias written though NULL was passed"
    assert bool(torch.isnan(ws[ws_n:]).all()), f"{tag}: ws written past its size function"
    return dw[GUARD:-GUARD].view(N, K), db[GUARD:-GUARD]


def wg_case(be, gh, gw, B, N, oracles, twice):
    M = B * gh * gw
    S = big_splits(M, N, K)
    G = min(64, M // 32)
    ws_n = wg_size(be, B, 16 * gh, 16 * gw, 16, N)
    assert ws_n == (S * N * K if S > 1 else 0) + G * N, (ws_n, S, G)
    for kind in oracles:
        tag = f"patch_wgrad {gh}x{gw} B{B} N{N} {kind}"
        g = be.gen(7919 * M + 31 * N + gw + (kind == "float"))
        px, do = wg_inputs(be, g, kind, B, gh, gw, N)
        dw, db = wg_call(be, B, gh, gw, N, px, do, ws_n, tag=tag)
        if kind in twice:
            dw2, db2 = wg_call(be, B, gh, gw, N, px, do, ws_n, tag=tag)
            assert torch.equal(bits(dw), bits(dw2)) and torch.equal(bits(db), bits(db2)), f"{tag}: the second call differs"
            dw3, _ = wg_call(be, B, gh, gw, N, px, do, ws_n, bias=False, tag=tag)
            assert torch.equal(bits(dw), bits(dw3)), f"{tag}: dW depends on dbias being asked for"
        Ad, Bd = do[:M].double().cpu(), unfolded(px[:B], gh, gw)
        exact, exact_b = Ad.t() @ Bd, Ad.sum(0)
        got, got_b = dw.float().cpu(), db.float().cpu()
        if kind == "exact":
            bad = got != exact.float().bfloat16().float()
            assert not bool(bad.any()), f"{tag}: {int(bad.sum())} of {bad.numel()} elements of dW differ from the exact product, first at {tuple(int(v) for v in bad.nonzero()[0])}"
            assert bool((got_b == exact_b.float().bfloat16().float()).all()), f"{tag}: dbias differs from the exact column sum"
        else:
            for name, gt, ex, E in (("dW", got, exact, 1.01 * (M + S) * 2.0 ** -24 * (Ad.abs().t() @ Bd.abs())),
                                    ("dbias", got_b, exact_b, 1.01 * (M + 8 + G) * 2.0 ** -24 * Ad.abs().sum(0))):
                err, bound = (gt.double() - ex).abs(), U * (ex.abs() + E) + E
                margin = float((err / bound.clamp_min(1e-300)).max())
                note(be, "perr", 0.0, f"{tag} {name} margin {margin:.3f}")
                assert bool((err <= bound).all()), f"{tag}: |{name} - exact| is {margin:.3f} x the bound U (|exact| + E) + E at its worst element"
            bf16_close(got, exact, tag, tol=WTOL, max_flip=MAX_FLIP)
            group_bias(got, exact, tag)


@pytest.mark.parametrize("backend,gh,gw,B,N", _params([c + (n,) for c in WG_CASES for n in (256, 512)], skip_emu=lambda r: r[2] >= 12 and r[3] == 512))
def test_patch_wgrad(backend, be, gh, gw, B, N):
    if be.name == "hip":
        oracles, twice = ("exact", "float"), ("exact", "float")
    else:
        oracles = ("exact", "float") if (gh, gw, B) in EMU_FLOAT and N == 256 else ("exact",)
        twice = ("exact",) if B < 12 else ()
    wg_case(be, gh, gw, B, N, oracles, twice)


@pytest.mark.parametrize("backend,gh,gw,B", _params([(2, 4, 4), (3, 5, 32), (8, 8, 3)]))
def test_patch_wgrad_selection(backend, be, gh, gw, B):
    N, M = 256, B * gh * gw
    ws_n = wg_size(be, B, 16 * gh, 16 * gw, 16, N)
    g = be.gen(M + gw)
    px, do = wg_inputs(be, g, "float", B, gh, gw, N)
    cols = unfolded(px[:B], gh, gw).float().bfloat16()
    for row, ch in ((0, 0), (M - 1, N - 1), (M // 2 + 1, 77)):
        do[:M] = 0
        do[row, ch] = 1.0
        dw, db = wg_call(be, B, gh, gw, N, px, do, ws_n, tag=f"selection {row},{ch}")
        assert torch.equal(bits(dw[ch].cpu()), bits(cols[row])), f"row {ch} of dW is not the pixels of patch {row}"
        rest = torch.ones(N, dtype=torch.bool)
        rest[ch] = False
        assert not bool(dw.float().cpu()[rest].any()), "a row of dW that no dout element selects is not zero"
        want_b = torch.zeros(N)
        want_b[ch] = 1.0
        assert torch.equal(db.float().cpu(), want_b)


def test_conv2d_order():
    """The oracle's (c, py, px) column order and (gy, gx) row order are nn.Conv2d's: its weight gradient from fp64 autograd."""
    g = torch.Generator().manual_seed(3)
    B, gh, gw, N = 2, 3, 5, 8
    px = torch.randn(B, 3, 16 * gh, 16 * gw, generator=g, dtype=torch.float64)
    w = torch.randn(N, 3, 16, 16, generator=g, dtype=torch.float64, requires_grad=True)
    bias = torch.zeros(N, dtype=torch.float64, requires_grad=True)
    do = torch.randn(B * gh * gw, N, generator=g, dtype=torch.float64)
    y = F.conv2d(px, w, bias, stride=16).flatten(2).transpose(1, 2).reshape(B * gh * gw, N)            # the model's token order
    gw_, gb_ = torch.autograd.grad(y, (w, bias), do)
    torch.testing.assert_close(do.t() @ unfolded(px, gh, gw), gw_.reshape(N, K), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(do.sum(0), gb_, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("backend", BACKENDS)
def test_patch_wgrad_rejects(backend, be):
    g = be.gen(13)
    B, gh, gw, N = 4, 4, 4, 256
    px, do = wg_inputs(be, g, "float", B, gh, gw, N)
    ws_n = wg_size(be, B, 64, 64, 16, N)
    assert ws_n > 0
    dw = torch.full((N * K + GUARD,), NAN, dtype=torch.bfloat16, device=be.dev)
    db = torch.full((N + GUARD,), NAN, dtype=torch.bfloat16, device=be.dev)
    ws = torch.full((ws_n + GUARD,), NAN, dtype=torch.float32, device=be.dev)
    ok = dict(B=B, H=64, W=64, Pp=16, N=N, px=px.data_ptr(), do=do.data_ptr(), dw=dw.data_ptr(), db=db.data_ptr(), ws=ws.data_ptr())

    def go(**ch):
        a = {**ok, **ch}
        return be.rc("vrwkv_patch_embed_wgrad_bf16", WG_T, a["B"], a["H"], a["W"], a["Pp"], a["N"], *(VP(a[k]) if a[k] else None for k in ("px", "do", "dw", "db", "ws")))

    def size(**ch):
        a = {**ok, **ch}
        return wg_size(be, a["B"], a["H"], a["W"], a["Pp"], a["N"])

    for bad in (dict(Pp=14, H=56, W=56), dict(N=128), dict(B=3), dict(W=24), dict(H=72), dict(N=384), dict(Pp=8)):
        assert go(**bad) == ESHAPE, bad
        assert size(**bad) == -1, bad
    assert size(B=3) == -1 and 3 * 16 == 48                         # B Mimg = 48
    assert go(B=0) == EINVAL and size(B=0) == -1
    for k in ("px", "do", "dw", "ws"):
        assert go(**{k: None}) == EINVAL, k
        assert go(**{k: ok[k] + 8}) == EALIGN, k
    assert all(bool(torch.isnan(t.float()).all()) for t in (dw, db, ws)), "a refused call wrote"
    assert go() == 0 and go(db=None) == 0                           # the same arguments without the fault are accepted
    assert bool(torch.isfinite(dw[:N * K].float()).all()) and bool(torch.isnan(dw[N * K:].float()).all())


# ------------------------------------------------------------------------------------------------ the tail
TAIL = [(1, 1, 64), (2, 16, 64), (3, 17, 128), (1, 16, 8192), (2, 600, 64), (5, 256, 512)]
EMU_BIG = ((1, 16, 8192), (2, 600, 64), (5, 256, 512))
FORMS = ("dense", "perm", "third", "sample")
EMU_BIG_PAIRS = (("dense", "plain"), ("perm", "delta"), ("third", "plain"), ("sample", "delta"))
FWD_T = [I] * 3 + [F32] + [VP] * 11
BWD_T = [I] * 3 + [VP] * 10
EXTRA = 7


def tail_ws(be, B, Lr, C):
    f = be.lib.vrwkv_ln_scatter_mean_ws_floats
    f.argtypes, f.restype = [I] * 3, L
    return int(f(B, Lr, C))


def parts(Lr):
    return min(64, (Lr + 7) // 8)


def tail_fwd(be, shp, x, delta, w, b, idx, nrows):
    B, Lr, C = shp
    res = {"out": nan_rows(be, nrows, C), "pooled": nan_rows(be, B, C), "mean": nan_rows(be, B * Lr, 1, torch.float32), "rstd": nan_rows(be, B * Lr, 1, torch.float32)}
    if delta is not None:
        res["xn"] = nan_rows(be, B * Lr, C)
    used = tail_ws(be, B, Lr, C)
    assert used == max(B * parts(Lr) * C, min(B * Lr, LN_BWD_GRID) * 2 * C)
    ws = nan_ws(be, used, C)
    be.call("vrwkv_ln_scatter_mean_fwd_bf16", FWD_T, B, Lr, C, EPS, P(x), P(delta), P(w), P(b), P(idx), P(res.get("xn")), P(res["out"]), P(res["pooled"]),
            P(res["mean"]), P(res["rstd"]), P(ws))
    assert bool(torch.isnan(ws[used:]).all()), "forward: ws written past vrwkv_ln_scatter_mean_ws_floats"
    for k, v in res.items():
        assert bool(torch.isnan(v[-1].float()).all()), f"{k}: guard row written"
        if k != "out":
            assert bool(torch.isfinite(v[:-1].float()).all()), f"{k}: not finite"
    return res


def tail_bwd(be, shp, dout, idx, dpooled, xn, f, w):
    B, Lr, C = shp
    res = {"dx": nan_rows(be, B * Lr, C), "dwb": nan_rows(be, 2, C, torch.float32)}
    used = tail_ws(be, B, Lr, C)
    ws = nan_ws(be, used, C)
    be.call("vrwkv_ln_gather_mean_bwd_bf16", BWD_T, B, Lr, C, P(dout), P(idx), P(dpooled), P(xn), P(f["mean"]), P(f["rstd"]), P(w), P(res["dx"]), P(res["dwb"]), P(ws))
    assert bool(torch.isnan(ws[used:]).all()), "backward: ws written past vrwkv_ln_scatter_mean_ws_floats"
    for k, v in res.items():
        assert bool(torch.isfinite(v[:-1].float()).all()), f"{k}: not finite"
        assert bool(torch.isnan(v[-1].float()).all()), f"{k}: guard row written"
    return res


def _tail_rows():
    rows = []
    for s in TAIL:
        for f in FORMS:
            for c in ("plain", "delta"):
                rows.append(("x".join(map(str, s)), f, c))
    return rows


@pytest.mark.parametrize("backend,shape,form,cfg", _params(_tail_rows(), skip_emu=lambda r: tuple(map(int, r[0].split("x"))) in EMU_BIG and r[1:] not in EMU_BIG_PAIRS))
def test_ln_scatter_mean(backend, be, shape, form, cfg):
    shp = B, Lr, C = tuple(map(int, shape.split("x")))
    ntok = B * Lr
    trimmed = be.name == "emu" and shp in EMU_BIG
    g = be.gen(43 * ntok + C + len(form) + len(cfg))
    x, w, b = rnd(be, g, ntok, C), rnd(be, g, C, scale=0.5, shift=1.0), rnd(be, g, C, scale=0.3)
    delta = rnd(be, g, ntok, C, scale=0.5) if cfg == "delta" else None
    nrows = ntok + (0 if form == "dense" else EXTRA)
    dout, dpooled = rnd(be, g, nrows, C), rnd(be, g, B, C)
    idx = None
    if form != "dense":
        idx = torch.randperm(nrows, generator=torch.Generator().manual_seed(ntok))[:ntok].to(torch.int64)
        if form == "third":
            idx[::3] = -1
        elif form == "sample":
            idx[(B - 1) * Lr:] = -1
        idx = idx.to(be.dev)
    keep = idx >= 0 if idx is not None else torch.ones(ntok, dtype=torch.bool, device=be.dev)
    rows = idx[keep] if idx is not None else torch.arange(ntok, device=be.dev)
    tag = f"ln_scatter_mean/{shape}/{form}/{cfg}"

    def run():
        f = tail_fwd(be, shp, x, delta, w, b, idx, nrows)
        xn = f["xn"] if delta is not None else x
        r = {**f}
        for name, d, dp in (("both", dout, dpooled), ("dout", dout, None), ("dpooled", None, dpooled)):
            for k, v in tail_bwd(be, shp, d, idx, dp, xn, f, w).items():
                r[f"{k}/{name}"] = v
        return r

    r1 = run()
    if not trimmed:
        same_bits(r1, run())
    named = torch.zeros(nrows + 1, dtype=torch.bool, device=be.dev)
    named[rows] = True
    assert bool(torch.isfinite(r1["out"][named].float()).all()), f"{tag} out: not finite"
    assert bool(torch.isnan(r1["out"][~named].float()).all()), f"{tag}: a row that no index names was written"

    # fp64
    kc = keep.cpu()
    for name, use_d, use_p in (("both", True, True), ("dout", True, False), ("dpooled", False, True)):
        xd, wd, bd = f64([x.cpu(), w.cpu(), b.cpu()])
        xn = xd if delta is None else ste(xd + delta.cpu().double())
        y, st = ref_ln(xn, wd, bd)
        pooled = y.view(B, Lr, C).mean(1)
        loss = 0.0
        if use_d:
            loss = loss + (y[kc] * dout[rows].cpu().double()).sum()
        if use_p:
            loss = loss + (pooled * dpooled.cpu().double()).sum()
        loss.backward()
        if name == "both":
            if rows.numel():                        # a single sample that is dropped whole leaves no row of out to look at
                act(be, r1["out"][rows].cpu(), y[kc], f"{tag} out", guard=False)
            act(be, r1["pooled"].cpu(), pooled, f"{tag} pooled")
            if delta is not None:
                act(be, r1["xn"].cpu(), xn, f"{tag} xn")
            m, r = r1["mean"][:-1, 0].double().cpu(), r1["rstd"][:-1, 0].double().cpu()
            em = ((m - st["mean"]).abs() / (st["mean"].pow(2) + st["var"] + EPS).sqrt()).max()
            er = ((r - st["rstd"]).abs() / st["rstd"]).max()
            for kind, e in (("mean", float(em)), ("rstd", float(er))):
                note(be, "perr", e, f"{tag} {kind}")
                assert e < PERR[be.name], f"{tag} {kind}: worst row off by {e:.3e} (relative)"
        act(be, r1[f"dx/{name}"].cpu(), xd.grad, f"{tag} dx {name}")
        par(be, r1[f"dwb/{name}"][0], wd.grad, f"{tag} dw {name}")
        par(be, r1[f"dwb/{name}"][1], bd.grad, f"{tag} db {name}")

    # bit for bit: the compressor's tail with one row per window, the LayerNorm + scatter entries
    ix = idx if idx is not None else torch.arange(ntok, device=be.dev)
    s = {"out": nan_rows(be, nrows, C), "mean": nan_rows(be, ntok, 1, torch.float32), "rstd": nan_rows(be, ntok, 1, torch.float32)}
    if delta is not None:
        s["xn"] = nan_rows(be, ntok, C)
    be.call("vrwkv_ln_pool_scatter_fwd_bf16", [I] * 5 + [F32] + [VP] * 9, B, Lr, 0, Lr, C, EPS, P(x), P(delta), P(w), P(b), P(idx), P(s.get("xn")), P(s["out"]),
            P(s["mean"]), P(s["rstd"]))
    same_bits(s, r1)
    xin = r1["xn"] if delta is not None else x
    if delta is None:
        s = {"out": nan_rows(be, nrows, C), "mean": nan_rows(be, ntok, 1, torch.float32), "rstd": nan_rows(be, ntok, 1, torch.float32)}
        be.call("vrwkv_ln_scatter_fwd_bf16", [L, I, F32] + [VP] * 7, ntok, C, EPS, P(x), P(w), P(b), P(ix), P(s["out"]), P(s["mean"]), P(s["rstd"]))
        same_bits(s, r1)
    s = {"dx": nan_rows(be, ntok, C), "dwb": nan_rows(be, 2, C, torch.float32)}
    ws = nan_ws(be, be.ws("vrwkv_add_ln_ws_floats", ntok, C), C)
    be.call("vrwkv_ln_gather_bwd_bf16", [L, I] + [VP] * 9, ntok, C, P(dout), P(ix), P(xin), P(r1["mean"]), P(r1["rstd"]), P(w), P(s["dx"]), P(s["dwb"]), P(ws))
    same_bits(s, {"dx": r1["dx/dout"], "dwb": r1["dwb/dout"]})


@pytest.mark.parametrize("backend", BACKENDS)
def test_ln_scatter_mean_arguments(backend, be):
    """What the two entries refuse, by return code; nothing is launched, nothing written."""
    B, Lr, C = 2, 16, 64
    t = torch.zeros(B * Lr + 1, C, dtype=torch.float32, device=be.dev)
    outs = [torch.full((B * Lr + 1, C), float("nan"), dtype=torch.float32, device=be.dev) for _ in range(5)]
    outs.append(torch.full((tail_ws(be, B, Lr, C),), float("nan"), dtype=torch.float32, device=be.dev))
    p = P(t)
    o = [P(v) for v in outs]
    fwd = [B, Lr, C, EPS, p, p, p, p, None, o[0], o[1], o[2], o[3], o[4], o[5]]
    bwd = [B, Lr, C, p, None, p, p, p, p, p, o[0], o[1], o[5]]

    def rc(which, **ch):
        a = list(fwd if which == "fwd" else bwd)
        for k, v in ch.items():
            a[int(k[1:])] = v
        return be.rc("vrwkv_ln_scatter_mean_fwd_bf16" if which == "fwd" else "vrwkv_ln_gather_mean_bwd_bf16", FWD_T if which == "fwd" else BWD_T, *a)

    for which, required in (("fwd", (4, 6, 7, 10, 11, 12, 13, 14)), ("bwd", (6, 7, 8, 9, 10, 11, 12))):
        for c in (96, 8, 8256, 0):
            assert rc(which, a2=c) == ESHAPE, (which, "C", c)
        assert rc(which, a0=0) == EINVAL and rc(which, a1=0) == EINVAL, (which, "sizes")
        for k in required:
            assert rc(which, **{f"a{k}": None}) == EINVAL, (which, "NULL argument", k)
    assert rc("fwd", a9=None) == EINVAL, "delta without xn"
    assert rc("bwd", a3=None, a5=None) == EINVAL, "neither dout nor dpooled"
    assert tail_ws(be, B, Lr, 96) == -1 and tail_ws(be, 0, Lr, C) == -1 and tail_ws(be, B, 0, C) == -1
    assert all(bool(torch.isnan(v).all()) for v in outs), "a refused call wrote"
    assert rc("fwd", a5=None, a9=None) == 0 and rc("bwd", a3=None) == 0 and rc("bwd", a5=None) == 0
