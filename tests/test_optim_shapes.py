"""The optimizer kernels (csrc/fused_ops.hip: adamw_kernel behind vrwkv_adamw_step_bf16 and vrwkv_adamw_step_clip_bf16, sqnorm_bf16_kernel)
per element at their edges, through the C ABI, on two backends with the same test bodies: the host lockstep emulator
(tests/emu/emu_fused_ops.cpp compiles the .hip file whole: CPU tensors, no marker) and the product library (CUDA tensors, `gpu` marker).

AdamW.  One 4-element vector per thread, 256 threads a workgroup, ceil((n / 4) / 256) workgroups, no loop.  Reference: the kernel's formula
in fp64 on the same fp32 / bf16 inputs, the scalar parameters rounded to fp32 as the ABI passes them (1 / bc1 and 1 / sqrt(bc2) formed in
fp64 and rounded, as the host does).  Bounds, per element, u = 2^-24, gamma = 1.01, counted from the roundings on the longest path:
    m'      |err| <= KM u (b1 |m| + (1 - b1) |g|)              KM = 3 + RG      fl(1 - b1), its product with g, the sum
    v'      |err| <= KV u v'                                   KV = 4 + 2 RG    fl(1 - b2), two products with g, the sum (all terms >= 0)
    master  |err| <= u (|p'| + lr (KA A + 3 wd |p|))           A = (b1 |m| + (1 - b1) |g|) / bc1 / (sqrt(v' / bc2) + eps) >= |m-hat / den|
            KA = KM + (KV / 2 + 2 + 1 + 1) + 1 + 3 + 1 + 1 = KM + KV / 2 + 11: the error of m' (against ITS magnitude: m' may cancel), of the
            denominator (half of v's, a sqrtf allowed 2 u since the chip's is not promised correctly rounded, a product, a sum), the
            product with 1 / bc1, a division allowed 3 u, the sum with the decay term, the product with lr; the decay term has its own
            product and shares the last two; the final subtraction rounds once against |p'|.
    RG = 0 where grad_scale is a power of two (0.5 everywhere in the plain variant, the clip variant with factor 1 or clip = 0), else
    RG = 8: the clip factor's sqrtf (2 u), + 1e-6 (1 u), division (3 u), the product bf16 * scale (1 u) and one more for the product with
    inv_world; the factor min(1, clip / (sqrt(sq) inv_world + 1e-6)) of the reference is formed in fp64.
Exact: param == bf16(master after the call) in bits; 32 guard elements on both sides of master, m, v, grad and param are untouched (NaN
still), grad itself is unchanged; across the vector that holds wd_boundary - global_offset every element matches ITS reference (decayed
before the boundary, not decayed from it on) and misses the other one.

What each case (n, global_offset, wd_boundary) reaches:
    (4, 0, 2)             one thread of one workgroup; the boundary inside the only vector
    (1020, 7, 510)        255 vectors: thread 255 idle (shorter than a workgroup); local boundary 503 = 4 * 125 + 3, inside a vector
    (1028, 1000, 1001)    257 vectors: the second workgroup has one busy thread; the offset moves the boundary to local 1 (vector 0)
    (2052, 5, 5)          513 vectors, three workgroups, the last with one thread; boundary at the shard's start: nothing decays
    (2052, 5, 5000)       boundary behind the shard: everything decays
    (1024, 0, 1023)       exactly one workgroup; the boundary on the last element of the last vector
    (1048580, 3, 524290)  GPU only: 1025 workgroups, the last with one thread; boundary 524287 = 4 * 131071 + 3
Each with step 1 (m = v = 0), 7, 1000 (m = 0.01 randn, v = 1e-4 rand), wd 0.1 and 0, grad_scale 0.5, lr 3e-3, betas (0.9, 0.99), eps 1e-8,
master 0.02 randn, grad bf16 randn; the clip variant at (1020, 7, 510) and (2052, 5, 5000), steps 1 and 7, inv_world 0.5, with a device
sqnorm of 1.5^2 (norm 0.75 below clip 1: factor exactly 1), 36 (factor 1 / 3.000001) and 36 with clip = 0 (no clipping).
Refusals: n % 4 != 0 -> VRWKV_ESHAPE; n <= 0, step < 1, each NULL pointer, a NULL sqnorm -> VRWKV_EINVAL; nothing written.

sqnorm.  grid = min(ceil((n / 8) / 256), 2048) workgroups, grid-stride over 16-byte vectors, fmaf chain per thread, wave tree, four
partials, one atomicAdd per workgroup.
  exact   values in {-1, 0, 1}, out preset to 5: every partial is an integer below 2^24, so out == 5 + sum x^2 whatever the order.
          n = 8 (one vector), 2040 (255 threads), 2056 (a second workgroup with one thread), 2048 * 256 * 8 + 8 (the grid cap: thread 0 of
          workgroup 0 takes a second trip).  The last takes 4 - 5 s on the emulator and stays there: it is the only pass through the cap.
  float   3 randn at n = 2^20 + 8 (513 workgroups, one trip) against fp64, out preset to 0.  Derived: 8 fmaf + 6 tree levels + 2 sums of
          the four partials, then G = 513 atomic adds of about equal partials in some order, sum_k u S k / G = u S (G + 1) / 2:
          (16 + 257) 1.01 u = 1.6e-5 -- looser than the 1e-5 the present GPU test allows, so the test holds min(derived, 1e-5) = 1e-5.
  refusals: n % 8 != 0 -> VRWKV_ESHAPE; n <= 0, NULL x, NULL out -> VRWKV_EINVAL; out untouched.
Three NaN vectors lie behind x in every case.

Measured (VRWKV_TEST_NOTES=1 prints every figure and the running worst), largest error in units of u against the magnitudes above (master:
against |p'| + lr A + lr wd |p|), worst case over the module and the case that gave it:
  emulator   m 1.78 (n1020 step1000), v 1.79 (n2052 bnd5 step7), master 3.29 (n2052 bnd5 step7 wd0); clip variant with a factor below 1:
             m 1.81, v 2.83, master 3.96 (n2052 step7); sqnorm relative error 3.8e-7
  MI355X     m 1.90 (n1048580 step7), v 1.86 (n1048580 step1000), master 5.05 (n1048580 step7 wd0.1); clip variant m 1.97, v 3.11,
             master 2.51 (n2052); sqnorm relative error 2.9e-7 and 5.0e-7 in two runs (the order of the atomics)
  against KM 3, KV 4 (11 and 20 in the clip variant) and KA 16 on the update's share.  Every exact assertion held on both.
Run time: 9 s for the 15 emulator cases (the grid-cap sqnorm 4.2 s, everything else under 1.1 s), 2 s for the 16 MI355X cases.
"""
import numpy as np
import pytest
import torch

from tests.parity import NOTES
from tests.test_glue_shapes import F32, I, L, P, VP, Backend, bits

BACKENDS = ["emu", pytest.param("hip", marks=pytest.mark.gpu)]
HIP_ONLY = [BACKENDS[1]]
EINVAL, ESHAPE = -1, -2
GUARD = 32
NAN = float("nan")
u = 2.0 ** -24
GAMMA = 1.01
LR, B1, B2, EPS, WD, GS = 3e-3, 0.9, 0.99, 1e-8, 0.1, 0.5
ADAMW_T = [L] + [VP] * 5 + [F32] * 5 + [I, F32, L, L]
CLIP_T = [L] + [VP] * 5 + [F32] * 5 + [I, VP, F32, F32, L, L]
SQNORM_T = [L, VP, VP]
CASES = [(4, 0, 2), (1020, 7, 510), (1028, 1000, 1001), (2052, 5, 5), (2052, 5, 5000), (1024, 0, 1023)]
BIG_CASE = (1048580, 3, 524290)
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
        print(f"[optim] {be.name} {name}: {kind} {val:.3e}   (worst so far: " + ", ".join(f"{k} {v[0]:.3e} {v[1]}" for k, v in w.items()) + ")")


def f32(x):
    return float(np.float32(x))


def guarded(be, data):
    """`data` inside a NaN buffer of the same dtype with GUARD elements on both sides; returns (buffer, view of the payload)."""
    buf = torch.full((GUARD + data.numel() + GUARD,), NAN, dtype=data.dtype, device=be.dev)
    buf[GUARD:GUARD + data.numel()] = data
    return buf, buf[GUARD:GUARD + data.numel()]


def guards_intact(name, buf):
    assert bool(torch.isnan(buf[:GUARD].float()).all()) and bool(torch.isnan(buf[-GUARD:].float()).all()), f"{name}: a guard element was written"


def make_state(be, n, step, seed):
    g = be.gen(seed)
    p = 0.02 * torch.randn(n, generator=g, device=be.dev)
    grad = torch.randn(n, generator=g, device=be.dev).bfloat16()
    if step > 1:
        m = 0.01 * torch.randn(n, generator=g, device=be.dev)
        v = 1e-4 * torch.rand(n, generator=g, device=be.dev)
    else:
        m, v = torch.zeros(n, device=be.dev), torch.zeros(n, device=be.dev)
    return p, m, v, grad


def reference(p, m, v, grad, step, gscale, wd_vec):
    """The kernel's formula in fp64; gscale a Python float (fp64), wd_vec the per-element decay.  Returns (m', v', p', magnitudes)."""
    lr, b1, b2, eps = f32(LR), f32(B1), f32(B2), f32(EPS)
    ibc1 = f32(1.0 / (1.0 - b1 ** step))
    isbc2 = f32(1.0 / np.sqrt(1.0 - b2 ** step))
    p, m, v, g = p.double(), m.double(), v.double(), grad.double() * gscale
    m2 = b1 * m + (1.0 - b1) * g
    v2 = b2 * v + (1.0 - b2) * g * g
    den = v2.sqrt() * isbc2 + eps
    p2 = p - lr * (m2 * ibc1 / den + wd_vec * p)
    m_mag = b1 * m.abs() + (1.0 - b1) * g.abs()
    A = m_mag * ibc1 / den
    return m2, v2, p2, (m_mag, v2, p2.abs(), lr * A, lr * wd_vec * p.abs())


def adamw_case(be, n, off, bnd, step, wd, tag, clip=None):
    """One call.  clip = (sq, clip): the clip variant with inv_world 0.5 and a device sqnorm of sq."""
    p0, m0, v0, grad = make_state(be, n, step, 7 * n + step + int(wd * 10))
    k = bnd - off
    if 0 < k < n:                                   # weights of ordinary size around the boundary: the decay must show there (checked below)
        lo, hi = 4 * ((k - 1) // 4), min(n, 4 * (k // 4) + 4)
        p0[lo:hi] = 0.03 * (1 - 2 * (torch.arange(lo, hi, device=be.dev) % 2)).float()
    (mb, mv), (mmb, mmv), (vb, vv), (gb, gv) = (guarded(be, t) for t in (p0, m0, v0, grad))
    pb, pv = guarded(be, torch.full((n,), NAN, dtype=torch.bfloat16, device=be.dev))
    if clip is None:
        gscale, RG = GS, 0
        rc = be.rc("vrwkv_adamw_step_bf16", ADAMW_T, n, P(mv), P(mmv), P(vv), P(gv), P(pv), LR, B1, B2, EPS, wd, step, GS, off, bnd)
    else:
        sq, cl = clip
        sqn = torch.tensor([sq], dtype=torch.float32, device=be.dev)
        factor = min(1.0, f32(cl) / (np.sqrt(f32(sq)) * 0.5 + f32(1e-6))) if cl > 0 else 1.0
        gscale, RG = 0.5 * factor, (0 if factor == 1.0 else 8)
        rc = be.rc("vrwkv_adamw_step_clip_bf16", CLIP_T, n, P(mv), P(mmv), P(vv), P(gv), P(pv), LR, B1, B2, EPS, wd, step, P(sqn), 0.5, cl, off, bnd)
        assert float(sqn) == f32(sq), f"{tag}: sqnorm was written"
    assert rc == 0, (tag, rc)
    for name, buf in (("master", mb), ("m", mmb), ("v", vb), ("grad", gb), ("param", pb)):
        guards_intact(f"{tag} {name}", buf)
        assert bool(torch.isfinite(buf[GUARD:-GUARD].float()).all()), f"{tag} {name}: not finite"
    assert torch.equal(bits(gv), bits(grad)), f"{tag}: grad changed"
    assert torch.equal(bits(pv), bits(mv.bfloat16())), f"{tag}: param is not bf16(master)"
    decays = (off + torch.arange(n, device=be.dev)) < bnd
    wd32 = f32(wd)
    wd_vec = decays.double() * wd32
    m2, v2, p2, (m_mag, v_mag, p_mag, lrA, lrD) = reference(p0, m0, v0, grad, step, gscale, wd_vec)
    KM, KV = 3 + RG, 4 + 2 * RG
    KA = KM + KV / 2 + 11
    tiny = 1e-300
    rm = float(((mmv.double() - m2).abs() / (u * m_mag).clamp_min(tiny)).max())
    rv = float(((vv.double() - v2).abs() / (u * v_mag).clamp_min(tiny)).max())
    errp = (mv.double() - p2).abs()
    rp = float((errp / (u * (p_mag + lrA + lrD)).clamp_min(tiny)).max())
    sfx = "_clip" if RG else ""
    note(be, "m" + sfx, rm, tag)
    note(be, "v" + sfx, rv, tag)
    note(be, "master" + sfx, rp, tag)
    assert rm <= GAMMA * KM, f"{tag}: m is off by {rm:.2f} u (b1 |m| + (1 - b1) |g|), allowed {KM}"
    assert rv <= GAMMA * KV, f"{tag}: v is off by {rv:.2f} u v', allowed {KV}"
    boundp = GAMMA * u * (p_mag + KA * lrA + 3 * lrD)
    worst = float((errp / boundp.clamp_min(tiny)).max())
    assert bool((errp <= boundp).all()), f"{tag}: master is {worst:.2f} x its bound at the worst element ({rp:.2f} u)"
    # the vector that holds the boundary, element by element: its own reference, and not the other one
    if wd > 0 and 0 < k < n:
        _, _, p_other, _ = reference(p0, m0, v0, grad, step, gscale, (~decays).double() * wd32)
        for e in range(lo, hi):
            assert float(errp[e]) <= float(boundp[e]), f"{tag}: element {e} (boundary at {k}) misses its reference"
            assert abs(float(mv[e]) - float(p_other[e])) > 4 * float(boundp[e]), f"{tag}: element {e} (boundary at {k}) took the other side's weight decay"


@pytest.mark.parametrize("backend,n,off,bnd", _params(CASES) + _params([BIG_CASE], HIP_ONLY))
def test_adamw(backend, be, n, off, bnd):
    for step in (1, 7, 1000):
        for wd in (WD, 0.0):
            adamw_case(be, n, off, bnd, step, wd, f"adamw n{n} off{off} bnd{bnd} step{step} wd{wd}")


@pytest.mark.parametrize("backend,n,off,bnd", _params([CASES[1], CASES[4]]))
def test_adamw_clip(backend, be, n, off, bnd):
    for step in (1, 7):
        for name, clip in (("below", (2.25, 1.0)), ("above", (36.0, 1.0)), ("clip0", (36.0, 0.0))):
            adamw_case(be, n, off, bnd, step, WD, f"adamw_clip {name} n{n} off{off} bnd{bnd} step{step}", clip=clip)


@pytest.mark.parametrize("backend", _params([()]))
def test_adamw_rejects(backend, be):
    n = 64
    p0, m0, v0, grad = make_state(be, n, 7, 1)
    (mb, mv), (mmb, mmv), (vb, vv), (gb, gv) = (guarded(be, t) for t in (p0, m0, v0, grad))
    pb, pv = guarded(be, torch.full((n,), NAN, dtype=torch.bfloat16, device=be.dev))
    sqn = torch.tensor([4.0], dtype=torch.float32, device=be.dev)
    ptr = dict(master=mv.data_ptr(), m=mmv.data_ptr(), v=vv.data_ptr(), grad=gv.data_ptr(), param=pv.data_ptr(), sqnorm=sqn.data_ptr())

    def plain(n=n, step=7, **kw):
        a = {**ptr, **kw}
        return be.rc("vrwkv_adamw_step_bf16", ADAMW_T, n, *(VP(a[k]) for k in ("master", "m", "v", "grad", "param")), LR, B1, B2, EPS, WD, step, GS, 0, n)

    def clip(n=n, step=7, **kw):
        a = {**ptr, **kw}
        return be.rc("vrwkv_adamw_step_clip_bf16", CLIP_T, n, *(VP(a[k]) for k in ("master", "m", "v", "grad", "param")), LR, B1, B2, EPS, WD, step,
                     VP(a["sqnorm"]), 0.5, 1.0, 0, n)

    for go in (plain, clip):
        assert go(n=62) == ESHAPE and go(n=63) == ESHAPE and go(n=2) == ESHAPE
        assert go(n=0) == EINVAL and go(n=-4) == EINVAL
        assert go(step=0) == EINVAL and go(step=-1) == EINVAL
        for k in ("master", "m", "v", "grad", "param"):
            assert go(**{k: None}) == EINVAL, k
    assert clip(sqnorm=None) == EINVAL
    for buf, orig in ((mb, p0), (mmb, m0), (vb, v0)):
        assert torch.equal(bits(buf[GUARD:-GUARD]), bits(orig)), "a rejected call wrote to its state"
    assert bool(torch.isnan(pb.float()).all()), "a rejected call wrote param"
    assert plain() == 0 and bool(torch.isfinite(pv.float()).all())          # the same arguments without the fault are accepted


def sq_input(be, n, vals):
    """n bf16 values and three NaN vectors behind them."""
    x = torch.full((n + 24,), NAN, dtype=torch.bfloat16, device=be.dev)
    x[:n] = vals
    return x


def sqnorm_call(be, n, x, preset, tag):
    out = torch.full((1 + 2 * GUARD,), NAN, dtype=torch.float32, device=be.dev)
    out[GUARD] = preset
    rc = be.rc("vrwkv_sqnorm_bf16", SQNORM_T, n, P(x), VP(out.data_ptr() + 4 * GUARD))
    assert rc == 0, (tag, rc)
    assert bool(torch.isnan(out[:GUARD]).all()) and bool(torch.isnan(out[GUARD + 1:]).all()), f"{tag}: wrote beside out"
    return float(out[GUARD])


@pytest.mark.parametrize("backend,n", _params([8, 2040, 2056, 2048 * 256 * 8 + 8]))
def test_sqnorm_exact(backend, be, n):
    g = be.gen(n)
    vals = torch.randint(-1, 2, (n,), generator=g, device=be.dev)
    vals[-8:] = 1                                   # the last vector (the lone thread of the last workgroup / the second trip) counts for 8
    got = sqnorm_call(be, n, sq_input(be, n, vals.bfloat16()), 5.0, f"sqnorm exact n{n}")
    want = 5 + int((vals * vals).sum())
    assert want < 2 ** 24
    assert got == float(want), f"sqnorm n{n}: {got} != {want}"


@pytest.mark.parametrize("backend", _params([()]))
def test_sqnorm_float(backend, be):
    n = 2 ** 20 + 8
    g = be.gen(3)
    x = sq_input(be, n, (3 * torch.randn(n, generator=g, device=be.dev)).bfloat16())
    got = sqnorm_call(be, n, x, 0.0, "sqnorm float")
    ref = float(x[:n].double().pow(2).sum())
    G = (n // 8 + 255) // 256
    derived = GAMMA * u * (8 + 6 + 2 + (G + 1) / 2)
    rel = abs(got - ref) / ref
    note(be, "sqnorm_rel", rel, f"sqnorm float n{n}")
    assert rel <= min(derived, 1e-5), f"sqnorm: relative error {rel:.2e} (derived {derived:.2e}, held to 1e-5)"


@pytest.mark.parametrize("backend", _params([()]))
def test_sqnorm_rejects(backend, be):
    x = sq_input(be, 64, torch.ones(64, dtype=torch.bfloat16, device=be.dev))
    out = torch.full((8,), NAN, dtype=torch.float32, device=be.dev)

    def go(n=64, x=x.data_ptr(), out=out.data_ptr()):
        return be.rc("vrwkv_sqnorm_bf16", SQNORM_T, n, VP(x), VP(out))

    assert go(n=60) == ESHAPE and go(n=7) == ESHAPE and go(n=65) == ESHAPE
    assert go(n=0) == EINVAL and go(n=-8) == EINVAL and go(x=None) == EINVAL and go(out=None) == EINVAL
    assert bool(torch.isnan(out).all()), "a rejected call wrote to out"
    out[0] = 0
    assert go() == 0 and float(out[0]) == 64.0 and bool(torch.isnan(out[1:]).all())
