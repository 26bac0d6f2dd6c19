"""The loss head (csrc/loss_fused.hip: ce_fwd, ce_bwd, ce_bwd_rows, head_dx, l2wrap_wgrad) per row and per element at its edges, through the
C ABI, on two backends with the same test bodies: the host lockstep emulator (tests/emu/emu_loss_fused.cpp compiles the .hip file whole: CPU
tensors, no marker) and the product library (CUDA tensors, `gpu` marker); and fused.head_loss / fused.loss_from_logits on the MI355X
(`gpu` marker only) against fp64.

Buffers, in every case: every output lies inside a NaN buffer with a guard row in front and behind (the int arg-max vector: -12345), ws is
NaN, sized by vrwkv_l2wrap_wgrad_ws_floats and followed by 32 guard floats, a NaN row lies behind every input matrix, and per-row inputs of
rows the kernel must not read are NaN.  After the call the outputs are finite and the guards untouched.

ce_fwd / ce_bwd / ce_bwd_rows.  One workgroup of 256 threads per row, 8 logits (16 bytes) per thread and trip.
  V      8 (one active thread), 2040 (thread 255 idle), 2048 (exactly one trip), 2056 (thread 0 takes a second trip), 4104 (a ragged second
         trip: 1 wave + 1 thread), 65536 (the real vocabulary, 32 trips)
  rows   (row_patterns; 16 .. 23 per V, in calls of 7 .. 10 rows so that a row which reads its neighbour shows) 2 randn; all equal
         (arg-max 0, lse = m + log V); +80 among -80 (the exponentials underflow, lse = 80, loss of that label 0); the maximum 12 over
         2 randn at 0, at V - 1, at each of the 8 slots of one 16-byte group, at 511 / 512 (last slot of lane 63, first of lane 64), at
         2047 / 2048 (first and second trip); two equal maxima in one 8-group, in two lanes of a wave, in two waves, in two trips of
         thread 0, at 0 and V - 1
  labels -100, 0, V - 1, the arg-max itself, V + 3 (forward only: loss 0); the backward covers arg == label and arg != label
  fwd    row_max == the fp64 max of the bf16 values, row_argmax == the smallest index attaining it (found explicitly), both exact;
         |lse - logsumexp64|, |loss - ref| <= K 2^-24 max(1, |lse|), K = 4 x the worst measured on the backend (below)
  bwd    row_w 0 (no label), 1 / (37 * 2) and 1; l2_factor 1e-4 / rows and 0.25.  A row with row_w = 0 has all bits 0 except at arg, where
         the value is bf16(fp32(max) * fp32(l2f)).  Labelled rows, per element against w (softmax - onehot) + [c = arg] max l2f in fp64:
             |got - ref| <= U (|ref| + E) + E,   U = 2^-8,   E = eps w p + 4 u (w |p - [c = label]| + [c = arg] |max l2f|) + 2^-126
             eps = 1.01 u (K max(1, |lse|) + 2 |x - lse| + 4),  u = 2^-24
         eps: exp(x - lse)'s argument carries the error of lse (K u max(1, |lse|)), the rounding of the difference (u |x - lse|) and of
         its product with log2 e inside the intrinsic (again u |x - lse|), each times the value; the intrinsic's own error is allowed 4 u.
         4 u: the fp32 roundings of the difference with the one-hot, the product with w, the product max * l2f and the sum.  2^-126: the
         smallest normal fp32, below which the chip may flush.  The elements at arg and at label are also asserted on their own.
  rows   ce_bwd_rows == the dense kernel's rows in bits for idx >= 0, zero bits for idx = -1; idx = a permutation with repeats and a -1
         (5 rows), all -1 (5 rows and 1 row), 256 random rows with -1 sprinkled in
  refusals: V % 8 != 0, V <= 0 -> VRWKV_ESHAPE; nrows <= 0, each NULL pointer -> VRWKV_EINVAL; outputs still NaN.

head_dx.  C 8, 2040, 2048, 2056 (thread 0's second trip), 4104; pos = a mix of >= 0, -1, -2; all -2; all -1 with dxc = NULL; two rows in
reversed compact order.  Exact (values; the kernel gives +0 where a product is -0): pos >= 0 the dxc row, -1
(c.float() * W[arg].float()).bfloat16() with c = bf16(max * l2f), -2 zeros.  row_max is NaN on every row that is not -1, negative on
two rows, 0 and 2e-38 (c rounds to 0) on two.

l2wrap_wgrad.  Tiles of 32 list positions, 8 columns a thread, 256 threads: C 8, 2048, 2056 (a second blockIdx.y with one thread), 4104.
  exact  x integers in [-4, 4], row_max in {0.5, 1, 2, 4}, l2f = 2^-8 (every coefficient a power of two), base dW integers in [-3, 3]:
         every product and partial sum is exact in fp32 in any order, so dW == (base.double() + S).float().bfloat16() at every element
         (the test first asserts that the fp64 total survives fp32).  Layouts (RUNS: run lengths in list order): singles; one run of
         70; 32 from a tile start; 32 mid-tile; a run ending at a tile end; 31 + 1; 33, 64, 65, 100 over 2, 3, 3, 4 tiles (middle tiles
         write Q and not P); two crossing runs back to back (tile 1 closes one into P and opens one into Q); n % 32 = 0, 1, 31;
         n = 1, 32, 33; a prefix srow[:n] that cuts a run; n = 0 (OK, nothing touched).  Rows of dW whose arg does not occur keep
         their bits; a second call on fresh copies is bit-identical.
  float  the oracle of test_emulated_head_loss.py::test_sparse_weight_gradient_groups_and_determinism (randn, its bound) at C = 2056.
  refusals: n < 0, NULL pointers -> VRWKV_EINVAL; C % 8 != 0, C <= 0 -> VRWKV_ESHAPE; the size function -1.

The host path on the MI355X (test_host_*): B 2, T 300 with pad 4, C 256, V 512, and one case at C 2056, V 520.  A common direction in the
unlabelled rows of x and in one row of W gives them all one arg-max (`one`: a run of ~540 positions over 17 tiles), or one per sample (`two`).  ~10 % labels
(compact, nrows = 256), no label at all (loss 0, dx == c W[arg] exactly, dW the sparse rows only), all labelled (dense fallback,
bit-equal to linear + loss_from_logits).  Reference: the bf16 logits F.linear(x, w) as given, the logit gradient in fp64 rounded once to
bf16, dx = dlog W and dW = dlog^T x in fp64; |dW - exact| <= 1.01 U (|G| + |exact|) + 1e-5 |dlog|^T |x| (G: the labelled rows' part),
|dx - exact| <= 1.01 U |exact| + 1e-5 |dlog| |W|, each plus one bf16 ulp, through the same products, of the few logit gradients whose
fp64 value lies within E of a rounding boundary (host_reference); test_head_loss_gpu.check on the same data.  loss_from_logits: the loss within
1.01 U |ref| + 1e-5 |ref| of fp64, the single nonzero of logits.grad on every w = 0 row by position and value.

Emulator thinning: none; every case of the C ABI runs on both backends (the 256-row ce_bwd_rows call too, 0.2 s at V = 65536).
Measured (VRWKV_TEST_NOTES=1 prints every figure and the running worst), worst case over the module and the case that gave it:
  emulator (host libm)   lse 0.95 x 2^-24 max(1, |lse|) (V2056 randn), loss 0.95 (the same row)  ->  K = 3.8;
                         logit gradient error / bound 0.992 (V2048 product-scale l2f, two maxima in two lanes: half a bf16 ulp);
                         sparse weight gradient, float oracle, error / bound 0.979
  MI355X (v_exp / v_log) lse 1.60 (V4104 all equal), loss 2.00 (V2056, maximum at slot 6 of a group)  ->  K = 8.0;
                         logit gradient error / bound 0.994 (V2056 product-scale l2f, randn); sparse weight gradient 0.977;
                         host path: dx error / bound 0.981 (two-all), dW 0.961 (two-some), 0 to 525 logit gradients of a case within E of a
                         rounding boundary; compact against dense dW rel-RMS 4.0e-5 .. 1.7e-4 under check's 1e-3
The exact oracles (row_max, row_argmax, the w = 0 rows, ce_bwd_rows, head_dx, the integer weight gradient) held at every element on both.
The no-label batch at C 256, V 512 was refused by the host path before this module (fused.wgrad_big_supported took a GEMM of 0 rows for
csrc/wgrad_big.h, whose size function answers -1: ValueError); it now takes the library product, which is all zeros.
Run time: 7 s for the 31 emulator cases (library build excluded, none above 0.8 s), 3 s for the 37 MI355X cases (none above 0.6 s).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.parity import NOTES
from tests.test_glue_shapes import F32, I, L, P, VP, Backend, bits

BACKENDS = ["emu", pytest.param("hip", marks=pytest.mark.gpu)]
EINVAL, ESHAPE = -1, -2
GUARD = 32
NAN = float("nan")
SENTINEL = -12345
u = 2.0 ** -24
U = 2.0 ** -8
GAMMA = 1.01
TINY = 2.0 ** -126
K_LSE = {"emu": 3.8, "hip": 8.0}           # 4 x the worst measured (module docstring)
HI = 12.0
VS = (8, 2040, 2048, 2056, 4104, 65536)
CS = (8, 2040, 2048, 2056, 4104)
L2W_CS = (8, 2048, 2056, 4104)
FWD_T = [L, I] + [VP] * 6
BWD_T = [L, I] + [VP] * 6 + [F32, VP]
ROWS_T = [L, I] + [VP] * 6 + [F32, VP, VP]
DX_T = [L, I] + [VP] * 5 + [F32, VP]
L2W_T = [L, I] + [VP] * 4 + [F32, VP, VP]
WORST = {b: {} for b in ("emu", "hip")}


def _params(items, backends=BACKENDS):
    out = []
    for b in backends:
        name, marks = (b, ()) if isinstance(b, str) else (b.values[0], b.marks)
        for it in items:
            it = it if isinstance(it, tuple) else (it,)
            out.append(pytest.param(name, *it, id="-".join(str(v) for v in (name,) + it), marks=marks))
    return out


@pytest.fixture
def be(request, backend):
    return Backend(request, backend)


def note(be, kind, val, name):
    w = WORST[be.name]
    if val > w.get(kind, (-1.0, ""))[0]:
        w[kind] = (val, name)
    if NOTES:
        print(f"[head] {be.name} {name}: {kind} {val:.3e}   (worst so far: " + ", ".join(f"{k} {v[0]:.3e} {v[1]}" for k, v in w.items()) + ")")


def f32(x):
    return float(np.float32(x))


def nan_t(be, *shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=be.dev)


def with_nan_row(be, t):
    """t (R, C) with one NaN row behind it; returns the (R + 1, C) allocation."""
    out = nan_t(be, t.shape[0] + 1, t.shape[1], dtype=t.dtype)
    out[:-1] = t
    return out


def out_rows(be, R, C, dtype=torch.bfloat16):
    """(R + 2, C) NaN: a guard row, R rows to write, a guard row."""
    return nan_t(be, R + 2, C, dtype=dtype)


def rows_written(name, buf):
    assert bool(torch.isfinite(buf[1:-1].float()).all()), f"{name}: not finite (unwritten, or NaN input was read)"
    assert bool(torch.isnan(buf[0].float()).all()) and bool(torch.isnan(buf[-1].float()).all()), f"{name}: a guard row was written"


# ------------------------------------------------------------------------------------------------ logit rows
def row_patterns(V):
    """(name, positions of the maximum) of every row pattern that fits V; None: no placed maximum."""
    g0 = 8 * min(V // 8 - 1, 37)
    pats = [("randn", None), ("equal", None), ("spike", None), ("randn_b", None), ("max@0", (0,)), ("max@V-1", (V - 1,))]
    pats += [(f"max@slot{e}", (g0 + e,)) for e in range(8)]
    if V >= 520:
        pats += [("max@511", (511,)), ("max@512", (512,))]
    if V >= 2056:
        pats += [("max@2047", (2047,)), ("max@2048", (2048,))]
    pats.append(("tie_group", (g0 + 5, g0 + 2)))
    if V >= 328:
        pats.append(("tie_lanes", (8 * 40 + 6, 8 * 3 + 1)))
    if V >= 808:
        pats.append(("tie_waves", (8 * 100 + 2, 8 * 10 + 4)))
    if V >= 2056:
        pats.append(("tie_trips", (2048 + 3, 5)))
    pats.append(("tie_ends", (V - 1, 0)))
    return pats


LABEL_KINDS = ("arg", "none", "zero", "last", "over")


def make_rows(be, V):
    """Every pattern of V: names, (R, V) bf16 logits, long labels, and the calls (lists of row numbers, 6 .. 10 each)."""
    g = be.gen(V)
    pats = row_patterns(V)
    R = len(pats)
    x = (2 * torch.randn(R, V, generator=g, device=be.dev)).bfloat16()
    labels = torch.empty(R, dtype=torch.long, device=be.dev)
    for r, (name, pos) in enumerate(pats):
        if name == "equal":
            x[r] = 1.5
        elif name == "spike":
            x[r] = -80.0
            x[r, V // 2] = 80.0
        elif pos is not None:
            for p in pos:
                x[r, p] = HI
        kind = "arg" if name == "spike" else LABEL_KINDS[r % 5]
        arg = int((x[r].double() == x[r].double().max()).nonzero()[0])
        labels[r] = {"arg": arg, "none": -100, "zero": 0, "last": V - 1, "over": V + 3}[kind]
    k = -(-R // 10)
    calls = [list(range(R))[i::k] for i in range(k)]          # interleaved: neighbours in a call are different patterns
    assert all(6 <= len(c) <= 10 for c in calls)
    return [p[0] for p in pats], x, labels, calls


def fwd_oracle(x, labels):
    """fp64 row_max, explicit first arg-max, logsumexp and loss of bf16 rows."""
    xd = x.double()
    m = xd.max(dim=1).values
    V = x.shape[1]
    idx = torch.arange(V, device=x.device).expand_as(xd)
    arg = torch.where(xd == m[:, None], idx, V).min(dim=1).values
    lse = torch.logsumexp(xd, dim=1)
    ok = (labels >= 0) & (labels < V)
    loss = torch.where(ok, lse - xd.gather(1, labels.clamp(0, V - 1)[:, None])[:, 0], torch.zeros_like(lse))
    return m, arg, lse, loss


def ce_fwd(be, x, labels, tag):
    """x (R, V), labels (R): the call with guarded buffers; returns loss, max, lse, arg (views of R rows)."""
    R, V = x.shape
    xa = with_nan_row(be, x)
    la = torch.cat([labels, torch.zeros(1, dtype=torch.long, device=be.dev)])
    fl = nan_t(be, 3, 3, R)                                     # loss / max / lse, each with a guard row on both sides
    ar = torch.full((3, R), SENTINEL, dtype=torch.int32, device=be.dev)
    rc = be.rc("vrwkv_ce_fwd_bf16", FWD_T, R, V, P(xa), P(la), P(fl[0, 1]), P(fl[1, 1]), P(fl[2, 1]), P(ar[1]))
    assert rc == 0, (tag, rc)
    for k, name in enumerate(("row_loss", "row_max", "row_lse")):
        assert bool(torch.isfinite(fl[k, 1]).all()), f"{tag} {name}: not finite"
        assert bool(torch.isnan(fl[k, 0]).all()) and bool(torch.isnan(fl[k, 2]).all()), f"{tag} {name}: a guard row was written"
    assert bool((ar[0] == SENTINEL).all()) and bool((ar[2] == SENTINEL).all()), f"{tag} row_argmax: a guard row was written"
    return fl[0, 1], fl[1, 1], fl[2, 1], ar[1]


@pytest.mark.parametrize("backend,V", _params(list(VS)))
def test_ce_fwd(backend, be, V):
    names, x, labels, calls = make_rows(be, V)
    for ci, rows in enumerate(calls):
        xr, lr = x[rows].contiguous(), labels[rows].contiguous()
        tag = f"ce_fwd V{V} call{ci}"
        loss, mx, lse, arg = ce_fwd(be, xr, lr, tag)
        m64, arg64, lse64, loss64 = fwd_oracle(xr, lr)
        for j, r in enumerate(rows):
            assert float(mx[j]) == float(m64[j]), f"{tag} {names[r]}: row_max {float(mx[j])} != {float(m64[j])}"
            assert int(arg[j]) == int(arg64[j]), f"{tag} {names[r]}: row_argmax {int(arg[j])} != {int(arg64[j])}"
        unit = u * lse64.abs().clamp_min(1.0)
        k_lse, k_loss = (lse.double() - lse64).abs() / unit, (loss.double() - loss64).abs() / unit
        for j, r in enumerate(rows):
            note(be, "K_lse", float(k_lse[j]), f"{tag} {names[r]}")
            note(be, "K_loss", float(k_loss[j]), f"{tag} {names[r]}")
            assert float(k_lse[j]) <= K_LSE[be.name], f"{tag} {names[r]}: lse off by {float(k_lse[j]):.2f} x 2^-24 max(1, |lse|)"
            assert float(k_loss[j]) <= K_LSE[be.name], f"{tag} {names[r]}: loss off by {float(k_loss[j]):.2f} x 2^-24 max(1, |lse|)"
            if names[r] == "spike":
                assert float(lse[j]) == 80.0 and float(loss[j]) == 0.0 and int(arg[j]) == V // 2
            if names[r] == "equal":
                assert int(arg[j]) == 0
            if int(lr[j]) >= V or int(lr[j]) < 0:
                assert float(loss[j]) == 0.0 and bits(loss[j:j + 1]).item() == 0, f"{tag} {names[r]}: a row without a label has a loss"


# ------------------------------------------------------------------------------------------------ logit gradient
def dlogits_ref(x, labels, w, mx32, lse64, arg, l2f):
    """fp64 w (softmax - onehot) + [c = arg] max l2f of bf16 rows, and the bound's E (module docstring).  mx32: the fp32 max (exact)."""
    R, V = x.shape
    xd = x.double()
    p = torch.exp(xd - lse64[:, None])
    cols = torch.arange(V, device=x.device)[None, :]
    onehot = (cols == labels[:, None]).double()
    at_arg = (cols == arg.long()[:, None]).double()
    wd = w.double()[:, None]
    l2 = (mx32.double() * f32(l2f))[:, None] * at_arg
    ref = wd * (p - onehot) + l2
    return ref, p, wd * (p - onehot).abs() + l2.abs()


def bwd_E(backend, x, w, p, mag, lse64):
    """The fp32 error allowed to one logit gradient before its bf16 rounding (module docstring)."""
    eps = GAMMA * u * (K_LSE[backend] * lse64.abs().clamp_min(1.0)[:, None] + 2 * (x.double() - lse64[:, None]).abs() + 4)
    return eps * w.double()[:, None] * p + 4 * u * mag + TINY


def bwd_bound(be, x, w, p, mag, lse64, ref):
    E = bwd_E(be.name, x, w, p, mag, lse64)
    return U * (ref.abs() + E) + E


def ce_bwd(be, x, labels, w, mx, lse, arg, l2f, tag):
    R, V = x.shape
    d = out_rows(be, R, V)
    xa, wa = with_nan_row(be, x), torch.cat([w, nan_t(be, 1)])
    la = torch.cat([labels, torch.zeros(1, dtype=torch.long, device=be.dev)])
    rc = be.rc("vrwkv_ce_bwd_bf16", BWD_T, R, V, P(xa), P(la), P(wa), P(mx), P(lse), P(arg), l2f, P(d[1]))
    assert rc == 0, (tag, rc)
    rows_written(tag, d)
    return d[1:-1]


def ce_bwd_rows(be, x, labels, w, mx, lse, arg, l2f, idx, tag):
    n, V = idx.numel(), x.shape[1]
    d = out_rows(be, n, V)
    xa, wa = with_nan_row(be, x), torch.cat([w, nan_t(be, 1)])
    la = torch.cat([labels, torch.zeros(1, dtype=torch.long, device=be.dev)])
    rc = be.rc("vrwkv_ce_bwd_rows_bf16", ROWS_T, n, V, P(xa), P(la), P(wa), P(mx), P(lse), P(arg), l2f, P(idx), P(d[1]))
    assert rc == 0, (tag, rc)
    rows_written(tag, d)
    return d[1:-1]


@pytest.mark.parametrize("backend,V,l2", _params([(V, l2) for V in VS for l2 in ("product", "quarter")]))
def test_ce_bwd(backend, be, V, l2):
    names, x, labels, calls = make_rows(be, V)
    labels = torch.where(labels >= V, torch.full_like(labels, -100), labels)      # a label >= V is defined for the forward only
    seen = set()
    for ci, rows in enumerate(calls):
        xr, lr = x[rows].contiguous(), labels[rows].contiguous()
        R = len(rows)
        l2f = 1e-4 / R if l2 == "product" else 0.25
        tag = f"ce_bwd V{V} {l2} call{ci}"
        _, mx, lse, arg = ce_fwd(be, xr, lr, tag)
        m64, arg64, lse64, _ = fwd_oracle(xr, lr)
        assert torch.equal(mx.double(), m64) and torch.equal(arg.long(), arg64)
        lab = lr >= 0
        scale = torch.tensor([1.0 / (37 * 2), 1.0], device=be.dev)[torch.arange(R, device=be.dev) % 2]
        w = torch.where(lab, scale, torch.zeros_like(scale)).float()
        d = ce_bwd(be, xr, lr, w, mx, lse, arg, l2f, tag)
        ref, p, mag = dlogits_ref(xr, lr, w, mx, lse64, arg, l2f)
        bound = bwd_bound(be, xr, w, p, mag, lse64, ref)
        err = (d.double() - ref).abs()
        coef = (mx * torch.tensor(f32(l2f), dtype=torch.float32, device=be.dev)).bfloat16()
        for j, r in enumerate(rows):
            name, a, lb = f"{tag} {names[r]}", int(arg[j]), int(lr[j])
            if float(w[j]) == 0.0:
                db = bits(d[j]).clone()
                assert int(db[a]) == int(bits(coef[j:j + 1])), f"{name}: the L2Wrap term at the arg-max is {float(d[j, a])}, not {float(coef[j])}"
                db[a] = 0
                assert int((db != 0).sum()) == 0, f"{name}: {int((db != 0).sum())} elements beside the arg-max are not +0"
                seen.add("w0")
                continue
            margin = float((err[j] / bound[j]).max())
            note(be, "dlogits_margin", margin, name)
            assert margin <= 1.0, f"{name}: |got - ref| is {margin:.3f} x its bound at element {int((err[j] / bound[j]).argmax())}"
            for c, what in ((a, "arg-max"), (lb, "label")):
                assert float(err[j, c]) <= float(bound[j, c]), f"{name}: the element at the {what} ({c}): {float(d[j, c])} against {float(ref[j, c])}"
            if l2 == "quarter" and a != lb:            # the L2Wrap term next to the soft-max term: it is really there
                assert abs(float(d[j, a]) - float(w[j] * p[j, a])) > 4 * float(bound[j, a]), f"{name}: no L2Wrap term on a labelled row"
            seen.add("arg==label" if a == lb else "arg!=label")
        if ci == 0:
            dense_bits = bits(d)
            g = be.gen(V + 1)
            for what, idx in (("perm", torch.tensor([R - 1, 0, -1, 0, 2 % R])), ("none5", torch.full((5,), -1)), ("none1", torch.full((1,), -1)),
                              ("rand256", torch.randint(-1, R, (256,), generator=g, device=be.dev).cpu())):
                idx = idx.to(be.dev).long().contiguous()
                dr = ce_bwd_rows(be, xr, lr, w, mx, lse, arg, l2f, idx, f"{tag} rows {what}")
                want = torch.where((idx >= 0)[:, None], dense_bits[idx.clamp(min=0)], torch.zeros_like(dense_bits[:1]))
                assert torch.equal(bits(dr), want), f"{tag} rows {what}: not the dense kernel's rows"
    assert seen == {"w0", "arg==label", "arg!=label"}, seen


@pytest.mark.parametrize("backend", _params([()]))
def test_ce_rejects(backend, be):
    R, V = 4, 64
    g = be.gen(5)
    x = with_nan_row(be, torch.randn(R, V, generator=g, device=be.dev).bfloat16())
    labels = torch.zeros(R + 1, dtype=torch.long, device=be.dev)
    w = torch.ones(R, device=be.dev)
    idx = torch.arange(R, device=be.dev)
    fl, ar, d = nan_t(be, 3, R), torch.full((R,), SENTINEL, dtype=torch.int32, device=be.dev), nan_t(be, R, V, dtype=torch.bfloat16)
    ptr = dict(x=x.data_ptr(), labels=labels.data_ptr(), loss=fl[0].data_ptr(), mx=fl[1].data_ptr(), lse=fl[2].data_ptr(), arg=ar.data_ptr(),
               w=w.data_ptr(), d=d.data_ptr(), idx=idx.data_ptr())

    def fwd(R=R, V=V, **kw):
        a = {**ptr, **kw}
        return be.rc("vrwkv_ce_fwd_bf16", FWD_T, R, V, *(VP(a[k]) for k in ("x", "labels", "loss", "mx", "lse", "arg")))

    def bwd(R=R, V=V, **kw):
        a = {**ptr, **kw}
        return be.rc("vrwkv_ce_bwd_bf16", BWD_T, R, V, *(VP(a[k]) for k in ("x", "labels", "w", "mx", "lse", "arg")), 0.25, VP(a["d"]))

    def rows(R=R, V=V, **kw):
        a = {**ptr, **kw}
        return be.rc("vrwkv_ce_bwd_rows_bf16", ROWS_T, R, V, *(VP(a[k]) for k in ("x", "labels", "w", "mx", "lse", "arg")), 0.25, VP(a["idx"]), VP(a["d"]))

    for go, ptrs in ((fwd, ("x", "labels", "loss", "mx", "lse", "arg")), (bwd, ("x", "labels", "w", "mx", "lse", "arg", "d")),
                     (rows, ("x", "labels", "w", "mx", "lse", "arg", "idx", "d"))):
        for V_bad in (60, 63, 4, 0, -8):
            assert go(V=V_bad) == ESHAPE, (go.__name__, V_bad)
        assert go(R=0) == EINVAL and go(R=-1) == EINVAL, go.__name__
        for k in ptrs:
            assert go(**{k: None}) == EINVAL, (go.__name__, k)
    assert bool(torch.isnan(fl).all()) and bool((ar == SENTINEL).all()) and bool(torch.isnan(d.float()).all()), "a rejected call wrote to an output"
    assert fwd() == 0 and bwd() == 0 and rows() == 0                           # the same arguments without the fault are accepted
    assert bool(torch.isfinite(fl).all()) and bool(torch.isfinite(d.float()).all())


# ------------------------------------------------------------------------------------------------ head_dx
DX_LAYOUTS = {
    "mix": [2, -1, -2, 0, -1, 1, -1, -1, -2],
    "all_pad": [-2] * 5,
    "all_unlabelled": [-1] * 6,
    "reversed": [1, 0],
}
DX_MAX = [-2.5, 0.0, -0.75, 2e-38, 3.0, 7.25, 11.0, 0.5, 5.0]           # dealt to the pos = -1 rows in order


@pytest.mark.parametrize("backend,C", _params(list(CS)))
def test_head_dx(backend, be, C):
    g = be.gen(C)
    Vw = 6
    W = with_nan_row(be, (0.05 * torch.randn(Vw, C, generator=g, device=be.dev)).bfloat16())
    l2f = 1e-4 / 9
    for name, pos_l in DX_LAYOUTS.items():
        tag = f"head_dx C{C} {name}"
        pos = torch.tensor(pos_l, dtype=torch.long, device=be.dev)
        n = pos.numel()
        ncomp = int((pos >= 0).sum())
        dxc = with_nan_row(be, torch.randn(ncomp, C, generator=g, device=be.dev).bfloat16()) if ncomp else None
        unl = (pos == -1).nonzero().flatten()
        mx = nan_t(be, n + 1)                                    # NaN wherever the kernel has no business reading
        mx[unl] = torch.tensor(DX_MAX[:unl.numel()], device=be.dev)
        arg = torch.full((n + 1,), 10 ** 6, dtype=torch.int32, device=be.dev)      # a wild row of W on rows that are not -1
        arg[unl] = torch.randint(0, Vw, (unl.numel(),), generator=g, device=be.dev).int()
        dx = out_rows(be, n, C)
        rc = be.rc("vrwkv_head_dx_bf16", DX_T, n, C, P(pos), P(dxc), P(W), P(mx), P(arg), l2f, P(dx[1]))
        assert rc == 0, (tag, rc)
        rows_written(tag, dx)
        got = dx[1:-1]
        want = torch.zeros(n, C, dtype=torch.bfloat16, device=be.dev)
        if ncomp:
            want[pos >= 0] = dxc[pos[pos >= 0]]
        c = (mx[unl] * torch.tensor(f32(l2f), device=be.dev)).bfloat16().float()
        want[unl] = (c[:, None] * W[arg[unl].long()].float()).bfloat16()
        bad = got.float() != want.float()
        assert not bool(bad.any()), f"{tag}: {int(bad.sum())} elements differ, first at {tuple(int(v) for v in bad.nonzero()[0])}"
        if unl.numel() >= 4:
            assert bool((c[:4] < 0).sum() == 2) and bool((c[:4] == 0).sum() == 2)


@pytest.mark.parametrize("backend", _params([()]))
def test_head_dx_rejects(backend, be):
    n, C = 3, 64
    g = be.gen(9)
    pos = torch.tensor([0, -1, -2], dtype=torch.long, device=be.dev)
    dxc, W = torch.randn(1, C, generator=g, device=be.dev).bfloat16(), torch.randn(4, C, generator=g, device=be.dev).bfloat16()
    mx, arg, dx = torch.ones(n, device=be.dev), torch.zeros(n, dtype=torch.int32, device=be.dev), nan_t(be, n, C, dtype=torch.bfloat16)
    ptr = dict(pos=pos.data_ptr(), dxc=dxc.data_ptr(), W=W.data_ptr(), mx=mx.data_ptr(), arg=arg.data_ptr(), dx=dx.data_ptr())

    def go(n=n, C=C, **kw):
        a = {**ptr, **kw}
        return be.rc("vrwkv_head_dx_bf16", DX_T, n, C, *(VP(a[k]) for k in ("pos", "dxc", "W", "mx", "arg")), 0.25, VP(a["dx"]))

    for C_bad in (60, 4, 0, -8):
        assert go(C=C_bad) == ESHAPE, C_bad
    assert go(n=0) == EINVAL and go(n=-1) == EINVAL
    for k in ("pos", "W", "mx", "arg", "dx"):
        assert go(**{k: None}) == EINVAL, k
    assert bool(torch.isnan(dx.float()).all()), "a rejected call wrote to dx"
    assert go() == 0 and bool(torch.isfinite(dx.float()).all())


# ------------------------------------------------------------------------------------------------ sparse L2Wrap weight gradient
RUNS = {
    # name: (run lengths in list order, n of the call or None for the whole list)
    "singles": ([1] * 40, None),
    "whole70": ([70], None),
    "run32_at_tile_start": ([32, 5], None),
    "run32_mid_tile": ([7, 32, 3], None),
    "ends_at_tile_end": ([10, 22, 4], None),
    "run31_plus_1": ([31, 1], None),
    "run33": ([3, 33, 2], None),
    "run64": ([5, 64, 1], None),
    "run65": ([2, 65, 4], None),
    "run100": ([1, 100, 3], None),
    "two_crossing": ([20, 30, 30, 5], None),
    "ragged0": ([32, 32], None),
    "ragged1": ([40, 25], None),
    "ragged31": ([50, 13], None),
    "n1": ([1], None),
    "n32": ([16, 16], None),
    "n32_one": ([32], None),
    "n33": ([33], None),
    "n33_two": ([20, 13], None),
    "prefix_cuts_run": ([10, 50, 20], 45),
}


def l2w_ws(be, n, C):
    f = be.lib.vrwkv_l2wrap_wgrad_ws_floats
    f.argtypes, f.restype = [L, I], L
    return int(f(n, C))


def l2w_case(be, g, runs, n, C, exact=True, l2f=2.0 ** -8):
    """A list of runs dealt to shuffled rows, three rows that are not listed (the labelled ones), the product's sort; returns everything
    the call and the oracle need."""
    total = sum(runs)
    n = total if n is None else n
    Vw = 2 * len(runs) + 3
    R = total + 3
    arg_sorted = torch.cat([torch.full((r,), 2 * k + 1) for k, r in enumerate(runs)])
    perm = torch.randperm(R, generator=g, device=be.dev).cpu()
    arg = torch.zeros(R, dtype=torch.int32)
    listed = torch.zeros(R, dtype=torch.bool)
    arg[perm[:total]] = arg_sorted.int()
    listed[perm[:total]] = True
    arg[perm[total:]] = 1                                        # unlisted rows share an arg with a listed run: only srow decides
    key = torch.where(listed, arg.long(), Vw)
    srow = torch.sort(key, stable=True).indices[:max(n, 1)].contiguous().to(be.dev)
    arg, listed = arg.to(be.dev), listed.to(be.dev)
    if exact:
        x = torch.randint(-4, 5, (R, C), generator=g, device=be.dev).bfloat16()
        mx = torch.tensor([0.5, 1.0, 2.0, 4.0], device=be.dev)[torch.randint(0, 4, (R,), generator=g, device=be.dev)]
        base = torch.randint(-3, 4, (Vw, C), generator=g, device=be.dev).bfloat16()
    else:
        x = torch.randn(R, C, generator=g, device=be.dev).bfloat16()
        mx = 10 * torch.rand(R, generator=g, device=be.dev) - 2
        base = (0.01 * torch.randn(Vw, C, generator=g, device=be.dev)).bfloat16()
    mx_in = torch.where(listed, mx, torch.full_like(mx, NAN))    # the max of an unlisted row is not to be read
    return dict(n=n, C=C, Vw=Vw, srow=srow, x=with_nan_row(be, x), mx=mx_in, arg=arg, base=base, l2f=l2f)


def l2w_call(be, c, tag):
    n, C = c["n"], c["C"]
    ws_n = l2w_ws(be, n, C)
    assert ws_n == 2 * ((n + 31) // 32) * C, (tag, ws_n)
    ws = nan_t(be, ws_n + GUARD)
    dW = out_rows(be, c["Vw"], C)
    dW[1:-1] = c["base"]
    rc = be.rc("vrwkv_l2wrap_wgrad_bf16", L2W_T, n, C, P(c["srow"]), P(c["x"]), P(c["mx"]), P(c["arg"]), c["l2f"], P(dW[1]), P(ws))
    assert rc == 0, (tag, rc)
    rows_written(tag, dW)
    assert bool(torch.isnan(ws[ws_n:]).all()), f"{tag}: ws written past vrwkv_l2wrap_wgrad_ws_floats"
    return dW[1:-1], ws


def l2w_sum(c):
    """S (Vw, C) in fp64 and the rows of dW that get nothing."""
    srow = c["srow"][:c["n"]]
    coef = (c["mx"] * torch.tensor(f32(c["l2f"]), device=c["mx"].device)).bfloat16().double()
    S = torch.zeros(c["Vw"], c["C"], dtype=torch.float64, device=srow.device)
    S.index_add_(0, c["arg"][srow].long(), coef[srow, None] * c["x"][srow].double())
    untouched = torch.ones(c["Vw"], dtype=torch.bool, device=srow.device)
    untouched[c["arg"][srow].long()] = False
    return S, untouched, coef


@pytest.mark.parametrize("backend,C", _params(list(L2W_CS)))
def test_l2wrap_wgrad_exact(backend, be, C):
    for li, (name, (runs, n)) in enumerate(RUNS.items()):
        tag = f"l2wrap C{C} {name}"
        c = l2w_case(be, be.gen(1000 * C + li), runs, n, C)
        got, _ = l2w_call(be, c, tag)
        again, _ = l2w_call(be, c, tag + " again")
        assert torch.equal(bits(got), bits(again)), f"{tag}: the second call differs"
        S, untouched, _ = l2w_sum(c)
        total = c["base"].double() + S
        assert torch.equal(total.float().double(), total), f"{tag}: the case is not exact in fp32"
        want = total.float().bfloat16()
        bad = got.float() != want.float()
        assert not bool(bad.any()), (f"{tag}: {int(bad.sum())} of {bad.numel()} elements differ from the exact sum, first at "
                                     f"{tuple(int(v) for v in bad.nonzero()[0])}")
        assert torch.equal(bits(got[untouched]), bits(c["base"][untouched])), f"{tag}: a row whose arg does not occur changed"
    # n = 0: accepted, nothing touched
    c = l2w_case(be, be.gen(C), [5], 0, C)
    got, ws = l2w_call(be, c, f"l2wrap C{C} n0")
    assert torch.equal(bits(got), bits(c["base"])) and bool(torch.isnan(ws).all()), "n = 0 wrote something"


@pytest.mark.parametrize("backend", _params([()]))
def test_l2wrap_wgrad_float(backend, be):
    """test_emulated_head_loss.py::test_sparse_weight_gradient_groups_and_determinism's data and bound at C = 2056: runs of 100, 28, 1 and 3 and
    single rows, the first 250 of the sorted list."""
    C, tag = 2056, "l2wrap float C2056"
    c = l2w_case(be, be.gen(11), [100, 28, 1, 3] + [1] * 168, 250, C, exact=False, l2f=1e-2)
    got, _ = l2w_call(be, c, tag)
    again, _ = l2w_call(be, c, tag + " again")
    assert torch.equal(bits(got), bits(again)), f"{tag}: the second call differs"
    S, untouched, coef = l2w_sum(c)
    G = c["base"].double()
    srow = c["srow"][:250]
    err = (got.double() - (G + S)).abs()
    tol = U * (G.abs() + (G + S).abs()) + 1e-6 * (coef[srow].abs().max() * c["x"][:-1].double().abs().max())
    note(be, "l2wrap_float_margin", float((err / tol).max()), tag)
    assert bool((err <= tol).all())
    assert torch.equal(bits(got[untouched]), bits(c["base"][untouched]))


@pytest.mark.parametrize("backend", _params([()]))
def test_l2wrap_wgrad_rejects(backend, be):
    C = 64
    c = l2w_case(be, be.gen(2), [40, 3], None, C)
    dW = c["base"].clone()
    ws = nan_t(be, l2w_ws(be, c["n"], C))
    ptr = dict(srow=c["srow"].data_ptr(), x=c["x"].data_ptr(), mx=c["mx"].data_ptr(), arg=c["arg"].data_ptr(), dW=dW.data_ptr(), ws=ws.data_ptr())

    def go(n=c["n"], C=C, **kw):
        a = {**ptr, **kw}
        return be.rc("vrwkv_l2wrap_wgrad_bf16", L2W_T, n, C, *(VP(a[k]) for k in ("srow", "x", "mx", "arg")), 2.0 ** -8, VP(a["dW"]), VP(a["ws"]))

    assert go(n=-1) == EINVAL
    for k in ptr:
        assert go(**{k: None}) == EINVAL, k
    for C_bad in (60, 4, 0, -8):
        assert go(C=C_bad) == ESHAPE, C_bad
        assert l2w_ws(be, 40, C_bad) == -1, C_bad
    assert l2w_ws(be, -1, C) == -1 and l2w_ws(be, 0, C) == 0 and l2w_ws(be, 33, C) == 4 * C
    assert torch.equal(bits(dW), bits(c["base"])) and bool(torch.isnan(ws).all()), "a rejected call wrote something"
    assert go() == 0 and not torch.equal(bits(dW), bits(c["base"]))


# ------------------------------------------------------------------------------------------------ the host path on the MI355X
def host_data(kind, targets, pad, C, V, seed):
    """x (B, T + pad, C) and W (V, C).  The rows without a label get a common direction that one row of W carries too -- the image-placeholder
    rows of a trained model, which all predict one token that the labelled rows do not: `one` gives them all the arg-max 7, `two` gives those
    of sample 0 the arg-max 7 and those of sample 1 the arg-max V - 212.  Their logit there is 2 (8 + N(0, 1)) + 0.8 N(0, 1), at least
    16 - 3.2 * 2.2 = 9 over 540 rows, against 0.8 * 3.5 + 0.4 for the largest of the others.
    (With the direction on the labelled rows too, their soft-max saturates at that token, row 7 holds most of dW's norm, and the second
    rounding of exactly that row -- bf16(bf16(G) + S), DESIGN.md -- puts the compact path 2.1e-3 rel-RMS from the dense one, above the 1e-3
    of test_head_loss_gpu.check, while every element stays within 0.81 of the fp64 bound: measured on the MI355X, not a case here.)"""
    B, T = targets.shape
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(B, T + pad, C, device="cuda", generator=g)
    W = 0.8 / C ** 0.5 * torch.randn(V, C, device="cuda", generator=g)        # logits of standard deviation 0.8 at every C
    d = F.normalize(torch.randn(2, C, device="cuda", generator=g), dim=1)
    unl = torch.zeros(B, T + pad, dtype=torch.bool, device="cuda")
    unl[:, pad:] = True
    unl[:, pad:T + pad - 1] = targets[:, 1:] < 0                              # row t predicts token t + 1; the last row has no target
    for b in range(B):
        x[b] += 8 * unl[b, :, None] * d[0 if kind == "one" else b % 2]
    W[7] += 2 * d[0]
    if kind == "two":
        W[V - 212] += 2 * d[1]
    return x.bfloat16(), W.bfloat16()


def host_targets(mode, B, T, V, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    ids = torch.randint(0, V, (B, T), device="cuda", generator=g)
    if mode == "all":
        return ids
    if mode == "none":
        return torch.full_like(ids, -100)
    keep = torch.rand(B, T, device="cuda", generator=g) < 0.1
    return torch.where(keep, ids, torch.full_like(ids, -100))


def host_run(x0, w0, targets, pad):
    """test_head_loss_gpu.run_both on given data: (loss, dx, dW) of linear + loss_from_logits and of head_loss, and the plan's pos."""
    from visualrwkv_amd import fused
    B, Tp, C = x0.shape
    head = torch.nn.Linear(C, w0.shape[0], bias=False, device="cuda", dtype=torch.bfloat16)
    with torch.no_grad():
        head.weight.copy_(w0)
    out = {}
    for mode in ("dense", "compact"):
        head.weight.grad = None
        x = x0.clone().requires_grad_(True)
        if mode == "dense":
            loss = fused.loss_from_logits(fused.linear(head, x)[:, pad:], targets, -100)
        else:
            plan = fused.HeadPlan(targets, pad)
            loss = fused.head_loss(head, x, plan)
            out["pos"] = plan.pos.view(B, Tp)
            out["n_lab"] = plan.n_labelled()
        loss.backward()
        torch.cuda.synchronize()
        out[mode] = (loss.detach(), x.grad.detach(), head.weight.grad.detach().clone())
    return out


def host_reference(x0, w0, targets, pad):
    """fp64 from the bf16 logits: loss, the logit gradient rounded once to bf16, dx, dW, the labelled rows' part G of dW, the products of
    absolute values for the bounds, and the per-row max / arg / labels."""
    B, Tp, C = x0.shape
    T, V = Tp - pad, w0.shape[0]
    N = B * Tp
    logits = F.linear(x0, w0).view(N, V)
    lab = torch.full((B, Tp), -100, dtype=torch.long, device="cuda")
    lab[:, pad:Tp - 1] = targets[:, 1:]
    real = torch.zeros(B, Tp, dtype=torch.bool, device="cuda")
    real[:, pad:] = True
    valid = (lab >= 0).sum(1).clamp(min=1)
    w = ((lab >= 0).float() / (valid.float().unsqueeze(1) * B)).view(N)
    lab, real = lab.view(N), real.view(N)
    m64, arg, lse64, loss64 = fwd_oracle(logits, lab)
    l2f = 1e-4 / (B * T)
    ref, p, mag = dlogits_ref(logits, lab, w, m64.float(), lse64, arg, l2f)
    E = bwd_E("hip", logits, w, p, mag, lse64)
    ref[~real] = 0
    dlog = ref.float().bfloat16().double()
    # Where the fp64 value lies within E of the middle between two bf16 numbers, a correct ce_bwd may round to either (test_ce_bwd holds it to
    # U (|ref| + E) + E): `slack` is one bf16 ulp on those elements, a handful in 300 000, and 0 everywhere else.  It enters the bounds of
    # dx and dW through the same products as dlog itself; without it one such element in a column of dW whose other terms cancel put all of
    # that row 24 x over 1e-5 |dlog|^T |x| on the dense and the compact path alike.
    ulp = torch.exp2(torch.frexp(dlog.abs().clamp_min(TINY))[1].double() - 8)
    slack = torch.where((ulp / 2 - (ref - dlog).abs() <= E) & real[:, None] & (dlog != 0), ulp, torch.zeros_like(ulp))
    xd, wd = x0.view(N, C).double(), w0.double()
    labelled = lab >= 0
    return dict(loss=float((loss64 * w.double()).sum()), dlog=dlog, dx=dlog @ wd, dW=dlog.t() @ xd, G=dlog[labelled].t() @ xd[labelled],
                absW=dlog.abs().t() @ xd.abs(), absx=dlog.abs() @ wd.abs(), slackW=slack.t() @ xd.abs(), slackx=slack @ wd.abs(),
                n_slack=int((slack != 0).sum()), mx=m64.float(), arg=arg, lab=lab, real=real, w=w, l2f=l2f)


def host_check(tag, out, ref, x0, w0):
    """The compact path's dx and dW (and the dense path's) against fp64, per element."""
    B, Tp, C = x0.shape
    for mode in ("compact", "dense"):
        loss, dx, dW = out[mode]
        assert abs(float(loss) - ref["loss"]) <= GAMMA * U * abs(ref["loss"]) + 1e-5 * abs(ref["loss"]), (tag, mode, float(loss), ref["loss"])
        err_x, bound_x = (dx.view(-1, C).double() - ref["dx"]).abs(), GAMMA * U * ref["dx"].abs() + 1e-5 * ref["absx"] + ref["slackx"] + TINY
        err_w, bound_w = (dW.double() - ref["dW"]).abs(), GAMMA * U * (ref["G"].abs() + ref["dW"].abs()) + 1e-5 * ref["absW"] + ref["slackW"] + TINY
        mx_, mw_ = float((err_x / bound_x).max()), float((err_w / bound_w).max())
        if NOTES:
            print(f"[head] hip {tag} {mode}: dx error / bound {mx_:.3f}, dW error / bound {mw_:.3f} ({ref['n_slack']} logit gradients may round either way)")
        assert mx_ <= 1.0, f"{tag} {mode}: dx is {mx_:.3f} x its bound at {tuple(int(v) for v in (err_x / bound_x == mx_).nonzero()[0])}"
        assert mw_ <= 1.0, f"{tag} {mode}: dW is {mw_:.3f} x its bound at {tuple(int(v) for v in (err_w / bound_w == mw_).nonzero()[0])}"


HOST_CASES = [
    # id, data, labels, (B, T, pad, C, V)
    ("one-some", "one", "some", (2, 300, 4, 256, 512)),
    ("two-some", "two", "some", (2, 300, 4, 256, 512)),
    ("one-none", "one", "none", (2, 300, 4, 256, 512)),
    ("two-all", "two", "all", (2, 300, 4, 256, 512)),
    ("one-some-wide", "one", "some", (2, 300, 4, 2056, 520)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("cid,data,mode,shape", [pytest.param(*c, id=c[0]) for c in HOST_CASES])
def test_host_head_loss(cid, data, mode, shape):
    from tests.test_head_loss_gpu import check
    B, T, pad, C, V = shape
    targets = host_targets(mode, B, T, V, seed=len(cid) + 1)
    x0, w0 = host_data(data, targets, pad, C, V, seed=len(cid))
    ref = host_reference(x0, w0, targets, pad)
    unl = ref["real"] & (ref["lab"] < 0)
    args = ref["arg"][unl].view(-1)
    shared = {7} if data == "one" else {7, V - 212}
    assert set(int(a) for a in args.unique()) == shared, f"{cid}: the data does not give the shared arg-max it was built for"
    out = host_run(x0, w0, targets, pad)
    n_lab = int((ref["lab"] >= 0).sum())
    assert out["n_lab"] == n_lab
    host_check(cid, out, ref, x0, w0)
    if mode == "all":                                  # the dense fallback: linear + loss_from_logits, bit for bit
        for a, b in zip(out["dense"], out["compact"]):
            assert torch.equal(a, b)
        return
    assert 0 <= n_lab <= 256 and (mode == "none") == (n_lab == 0)
    check(out, cid)
    if mode == "none":
        loss, dx, dW = out["compact"]
        assert float(loss) == 0.0
        c = (ref["mx"] * torch.tensor(f32(ref["l2f"]), device="cuda")).bfloat16().float()
        want = (c[:, None] * w0[ref["arg"]].float()).bfloat16().float()
        want[~ref["real"]] = 0
        assert torch.equal(dx.view(-1, C).float(), want), "without a label dx is c W[arg] on the real rows and 0 on the pad rows"
        other = torch.ones(V, dtype=torch.bool, device="cuda")
        other[list(shared)] = False
        assert not bool(dW[other].any()), "without a label only the arg-max rows of dW are nonzero"
        assert bool((dW[7] != 0).any())


@pytest.mark.gpu
def test_host_loss_from_logits():
    """fused.loss_from_logits alone: the loss against fp64, and on every row without a label the single nonzero of logits.grad by position
    and value -- four to five orders below the soft-max gradient of the labelled rows, so a relative RMS over the gradient cannot see it."""
    from visualrwkv_amd import fused
    B, T, C, V = 2, 300, 256, 512
    targets = host_targets("some", B, T, V, seed=4)
    x0, w0 = host_data("two", targets, 0, C, V, seed=3)
    ref = host_reference(x0, w0, targets, 0)
    logits = F.linear(x0, w0).detach().requires_grad_(True)
    loss = fused.loss_from_logits(logits, targets, -100)
    loss.backward()
    torch.cuda.synchronize()
    assert abs(float(loss.detach()) - ref["loss"]) <= GAMMA * U * abs(ref["loss"]) + 1e-5 * abs(ref["loss"]), (float(loss.detach()), ref["loss"])
    grad = logits.grad.view(B * T, V)
    w0rows = (ref["w"] == 0).nonzero().flatten()
    assert w0rows.numel() > 400
    coef = (ref["mx"] * torch.tensor(f32(ref["l2f"]), device="cuda")).bfloat16()
    g0 = grad[w0rows]
    at = g0.gather(1, ref["arg"][w0rows][:, None])[:, 0]
    assert torch.equal(bits(at), bits(coef[w0rows])), "the L2Wrap term of a row without a label is not bf16(max * 1e-4 / (B T)) at its arg-max"
    assert bool((at > 0).all())
    assert int((bits(g0) != 0).sum()) == w0rows.numel(), "a row without a label has more than one nonzero (or a -0) in its logit gradient"
    lab = ref["w"] > 0
    err = (grad[lab].double() - ref["dlog"][lab]).abs()
    assert bool((err <= 2 * U * ref["dlog"][lab].abs() + 1e-9).all())          # the labelled rows: one bf16 ulp of the once-rounded fp64 gradient
