"""The two weight-gradient kernels (csrc/lora_wgrad.hip: lora_wgrad.h for the LoRA factors, wgrad_big.h for r / k / v / o and the channel
mix) at their slice, stage and tile edges, through the C ABI, on two backends with the same test bodies: the host lockstep emulator
(tests/emu/emu_lora_wgrad.cpp compiles the .hip file whole, so splits(), big_splits(), the D / 16 switch, the ws contracts, the reduce grid
cap and the argument checks are the product's own: CPU tensors, no marker) and the product library (CUDA tensors, `gpu` marker).  The
emulator's vmem_wait is a no-op: the LDS-DMA waits and barriers of wgrad_big_kernel's ring are tested on the MI355X only.

Oracles (both in every case unless the case says otherwise; C = A^T B, A (M x N1) and B (M x N2) bf16):
  exact  Inputs are integers, uniform in [-8, 8], stored as bf16.  Every product (|.| <= 64) and every partial sum (M <= 262 144: below
         2^24) is an integer that fp32 holds exactly, in any summation order, so the result has to EQUAL
         (A.double().T @ B.double()).float().bfloat16() at every element, no tolerance: one dropped, doubled or misplaced product among
         thousands fails.  Values are compared, not bit patterns: a lone row gives -0 in fp64 where the kernel's 0 + (-0) gives +0.
  float  Inputs are randn (x 0.3 for A / Wide, x 0.5 for B / Narrow, the scales of tests/test_fused_gpu.py).  Per element
             |out - exact| <= U (|exact| + E) + E,     U = 2^-8,     E = 1.01 (M + S) 2^-24 (|A|^T |B|)
         E is the textbook bound of an fp32 sum of M exact products plus S partials in ANY order (gamma_n <= 1.01 n u for n u < 0.01,
         u = 2^-24), U the unit roundoff of bf16 (8 significant bits, round to nearest: half an ulp of a value just above a power of
         two), applied to the fp32 sum, which is within E of the exact one.  Derived, not measured; a correct result reaches 0.995 of it.
         Also tests.parity.bf16_close(tol=1e-3, max_flip=0.02), the figures test_big_weight_gradient_against_fp32 asserts, and group_bias.
Asserted in every case: return code 0; `out` lies inside a larger NaN buffer with 32-element guards on both sides, ws is NaN and followed
by a 32-float guard: out finite, guards untouched; rows M .. M+2 of both input allocations are NaN (an over-read of a ragged tail poisons
the result); a second call on the same inputs is bit-identical.  ws is sized by the library's own *_ws_floats.

What each shape reaches.
  skinny, C ABI, both backends (test_skinny): Nw = 128 gives splits() = steps, every slice one step, S = steps
    D    32, 64, 96, 128, 160, 256    wgrad_kernel<2>, <4>, <6>, <8>, <10>, two column groups of <8>; chunks per thread NL = 1, 1, 2, 2, 3, 2;
                                      a partial `q < NCH` trip at 32 (128 of 256 threads), 96 (384 of 512), 160 (640 of 768)
    M    1, 31, 32, 33, 97, 289       less than one step; ragged by 31 and by 1; S = 1, 1, 1, 2, 4, 10
    M    32 steps - 7, steps 1, 2, 3, 4, 5, 7, 8, 9, 13      reduce_kernel's loop unrolled by 4 and every remainder, up to three trips
    transposed 0 and 1 at every (D, M)
  test_skinny_odd_blocks: Nw = 384 with D = 96 and D = 256: three column blocks; `blockIdx.x % ngrp`, `/ ngrp` with two groups
  test_skinny_splits: Nw = 32 896, D = 256, M = 32: 512 / 257 = 0 slices clamped to 1 (`s < 1`);  Nw = 8192, D = 96, M = 613: s = 8 < 20
    steps, slices of 2 and 3 steps, the last ragged -- the only pass through `s < nsteps` on the emulator
  test_skinny_multistep (GPU only, product path): Nw = 2048 (s = 32; 16 for D = 256), every D, both orientations, steps = s + 1 (one slice
    of 2 steps), 2.5 s with a ragged last step (slices of 2 and 3), 4.5 s (4 and 5)
  test_skinny_slices (emulator only, emu_wgrad_skinny_slices: the product's launch<ND> with a caller-chosen S): Nw = 128, every D, both
    orientations, (steps, S) = (5, 1), (6, 1), (5, 2), (7, 2), (9, 2), (11, 3) at M = 32 steps and 32 steps - 31: odd and even slice
    lengths, the `t + 1 < t1` guard, the fetches that run past the slice and past M
  big, C ABI, both backends:
    test_big_stages: 256 x 256 (one tile, S = min(8, M / 32)) at M / 32 = 1, 2, 7, 8, 12, 20, 28, 36, 44, 52, 60, 68, 76, 84, 92: stages
      per slice 1 (prologue with one request, drain), 2 (two requests, `ns < STAGES`), 3, 4 (tail only), 5 .. 7 (one steady group, tails
      of 2, 3, 4), 8 .. 10 (two groups), 11, 12 (three groups); from 20 on every launch mixes two neighbouring lengths
    test_big_tiles: (512, 256), (256, 512), (768, 512) at M / 32 = 8, 20: i1 / i2 / sl with T1 != T2, S = 8, 8, 6 (43 tiles short of 256)
    test_big_reduce_cap: 3072 x 2816 at M = 64: 132 tiles, S = 2, a reduce grid of 8448 capped to 8192 (256 workgroups take a second trip)
    test_big_large (GPU only): 4096 x 4096 at M / 32 = 1, 4, 5, 9 (256 tiles, S = 1: the bf16 epilogue after long slices, no scratch),
      2048 x 2048 at M = 288 (S = 4), 2048 x 4096 at M = 160 (S = 2)
  test_rejects_skinny / test_rejects_big: the exact VRWKV_E* code, -1 from the size function, NaN outputs untouched, on both backends.

What the emulator does not assert (plan() below; with everything it took 374 s, the module has to stay near 150 s).  The MI355X runs both
oracles and the repeated call in every case.  The emulator runs the exact oracle in every case that is not GPU-only, and
  - the float oracle (bound, bf16_close, group_bias) at M = 1, 33, 409 of test_skinny, M = 33 of test_skinny_odd_blocks, S = 3 of
    test_skinny_slices, M / 32 = 1, 8, 20 of test_big_stages and M / 32 = 8 of test_big_tiles, not in test_skinny_splits and
    test_big_reduce_cap: its index math is the exact oracle's, its fp32 arithmetic the host's and not the chip's;
  - the repeated call with the exact oracle only, and not in test_skinny_splits, test_big_reduce_cap, test_big_tiles, test_big_stages from
    M / 32 = 20 on and the unragged M of test_skinny_slices: one workgroup at a time in a fixed order has no other order to take;
  - test_skinny_splits in one orientation per shape, test_skinny_slices in one per M (the orientation only reaches reduce_kernel).

Measured (VRWKV_TEST_NOTES=1 prints every figure and the running worst).  Float oracle, worst case over the module:
  emulator   flips 3.3e-4 (skinny D96 M409 tr0), rel-RMS 2.6e-5 (big 768x512 M256), largest error / bound 0.994 (big 256x256 M32)
  MI355X     flips 2.4e-4 (skinny D32 M33 tr0), rel-RMS 6.6e-5 (skinny D128 M153 tr1), largest error / bound 0.995 (skinny Nw32896 D256
             M32 tr1): a bf16 rounding of half an ulp just above a power of two, E contributes nothing visible
  against limits of 0.02 and 1e-3.  The exact oracle held at every element of every case on both backends.
Run time: 121 s for the 147 emulator cases (library build excluded; the slowest: test_skinny_splits 14 s and 10 s, test_big_reduce_cap
11 s, everything else under 6 s), 5.4 s for the 142 MI355X cases (the slowest 0.7 s).
"""
import pytest
import torch

from tests.parity import NOTES, bf16_close, group_bias
from tests.test_glue_shapes import I, L, P, VP, Backend, bits

BACKENDS = ["emu", pytest.param("hip", marks=pytest.mark.gpu)]
EINVAL, ESHAPE, EALIGN = -1, -2, -3
GUARD = 32                      # NaN elements on both sides of out and behind ws
U = 2.0 ** -8
TOL, MAX_FLIP = 1e-3, 0.02      # tests/test_fused_gpu.py::test_big_weight_gradient_against_fp32
NAN = float("nan")

SKINNY_D = (32, 64, 96, 128, 160, 256)
SKINNY_M = (1, 31, 32, 33, 97, 289) + tuple(32 * s - 7 for s in (1, 2, 3, 4, 5, 7, 8, 9, 13))
EMU_FLOAT_M = (1, 33, 409)      # where the emulator runs the float oracle too (module docstring)
SLICES = ((5, 1), (6, 1), (5, 2), (7, 2), (9, 2), (11, 3))          # (steps, S) of emu_wgrad_skinny_slices
BIG_STAGES_M32 = (1, 2, 7, 8, 12, 20, 28, 36, 44, 52, 60, 68, 76, 84, 92)
BIG_TILES = ((512, 256), (256, 512), (768, 512))
BIG_LARGE = ((4096, 4096, 32), (4096, 4096, 128), (4096, 4096, 160), (4096, 4096, 288), (2048, 2048, 288), (2048, 4096, 160))
WORST = {b: {"flip": (0.0, ""), "rms": (0.0, ""), "margin": (0.0, "")} for b in ("emu", "hip")}


def _params(items, backends=BACKENDS):
    out = []
    for b in backends:
        name, marks = (b, ()) if isinstance(b, str) else (b.values[0], b.marks)
        for it in items:
            it = it if isinstance(it, tuple) else (it,)
            out.append(pytest.param(name, *it, id="-".join(str(v) for v in (name,) + it), marks=marks))
    return out


HIP_ONLY = [BACKENDS[1]]


@pytest.fixture
def be(request, backend):
    return Backend(request, backend)


def rc_of(be, fn, argtypes, *args):
    f = getattr(be.lib, fn)
    f.argtypes, f.restype = argtypes + [VP], I
    return f(*args, be.stream)


def size_of(be, fn, *args):
    f = getattr(be.lib, fn)
    f.argtypes, f.restype = [L, I, I], L
    return int(f(*args))


SKINNY_T = [L, I, I, VP, VP, VP, I, VP]
BIG_T = [L, I, I, VP, VP, VP, VP]


def operand(be, g, kind, M, N, scale):
    """(M + 3, N) bf16: M rows of integers in [-8, 8] (`exact`) or of scale * randn (`float`), then three rows of NaN."""
    t = torch.full((M + 3, N), NAN, dtype=torch.bfloat16, device=be.dev)
    if kind == "exact":
        t[:M] = torch.randint(-8, 9, (M, N), generator=g, device=be.dev).bfloat16()
    else:
        t[:M] = (torch.randn(M, N, generator=g, device=be.dev) * scale).bfloat16()
    return t


def note(be, kind, val, name):
    if val > WORST[be.name][kind][0]:
        WORST[be.name][kind] = (val, name)
    if NOTES:
        w = WORST[be.name]
        print(f"[wgrad] {be.name} {name}: {kind} {val:.3e}   (worst so far: " + ", ".join(f"{k} {v[0]:.3e} {v[1]}" for k, v in w.items()) + ")")


def plan(be, floats=True, twice=True):
    """(oracles, the oracles whose call is repeated) of a case: everything on the MI355X; on the emulator the float oracle where `floats`
    and the repeated call where `twice` (module docstring: what the emulator leaves to the GPU)."""
    if be.name == "hip":
        return ("exact", "float"), ("exact", "float")
    return ("exact", "float") if floats else ("exact",), ("exact",) if twice else ()


def run_case(be, tag, M, n1, n2, launch, ws_n, S, transposed=0, todo=(("exact", "float"), ("exact", "float")), seed=0):
    """launch(A, B, out_address, ws) -> return code, for C (n1 x n2) = A^T B (stored transposed if `transposed`), A (M x n1), B (M x n2);
    todo: see plan()."""
    oracles, twice = todo
    for kind in oracles:
        g = be.gen(1000003 * seed + 7919 * M + 31 * n1 + n2 + (kind == "float"))
        A, B = operand(be, g, kind, M, n1, 0.3), operand(be, g, kind, M, n2, 0.5)
        name = f"{tag} {kind}"
        bufs = []
        for rep in range(2 if kind in twice else 1):
            buf = torch.full((GUARD + n1 * n2 + GUARD,), NAN, dtype=torch.bfloat16, device=be.dev)
            ws = torch.full((ws_n + GUARD,), NAN, dtype=torch.float32, device=be.dev)
            rc = launch(A, B, buf.data_ptr() + 2 * GUARD, ws)
            assert rc == 0, (name, rc)
            assert bool(torch.isfinite(buf[GUARD:-GUARD].float()).all()), f"{name}: out is not finite (unwritten, or NaN rows / scratch were read)"
            assert bool(torch.isnan(buf[:GUARD].float()).all()) and bool(torch.isnan(buf[-GUARD:].float()).all()), f"{name}: a guard of out was written"
            assert bool(torch.isnan(ws[ws_n:]).all()), f"{name}: ws written past its *_ws_floats"
            bufs.append(buf)
        assert torch.equal(bits(bufs[0][GUARD:-GUARD]), bits(bufs[-1][GUARD:-GUARD])), f"{name}: the second call differs"
        Ad, Bd = A[:M].double(), B[:M].double()
        exact = Ad.t() @ Bd
        got = bufs[0][GUARD:-GUARD].view((n2, n1) if transposed else (n1, n2))
        got = (got.t() if transposed else got).float()
        if kind == "exact":
            want = exact.float().bfloat16().float()
            bad = got != want
            assert not bool(bad.any()), (f"{name}: {int(bad.sum())} of {bad.numel()} elements differ from the exact product, first at "
                                         f"{tuple(int(v) for v in bad.nonzero()[0])}")
        else:
            E = 1.01 * (M + S) * 2.0 ** -24 * (Ad.abs().t() @ Bd.abs())
            err, bound = (got.double() - exact).abs(), U * (exact.abs() + E) + E
            margin = float((err / bound.clamp_min(1e-300)).max())
            note(be, "margin", margin, name)
            assert bool((err <= bound).all()), f"{name}: |out - exact| is {margin:.3f} x the bound U (|exact| + E) + E at its worst element"
            rms, flip = bf16_close(got, exact, name, tol=TOL, max_flip=MAX_FLIP)
            note(be, "rms", rms, name)
            note(be, "flip", flip, name)
            group_bias(got, exact, name)


# ------------------------------------------------------------------------------------------------ skinny
def skinny_case(be, M, Nw, D, transposed, tag, want_S=None, todo=(("exact", "float"), ("exact", "float"))):
    ws_n = size_of(be, "vrwkv_wgrad_skinny_ws_floats", M, Nw, D)
    assert ws_n > 0 and ws_n % (Nw * D) == 0, (tag, ws_n)
    S = ws_n // (Nw * D)
    if want_S is not None:
        assert S == want_S, f"{tag}: splits() gave {S} slices, the case is written for {want_S}"

    def launch(wide, narrow, out, ws):
        return rc_of(be, "vrwkv_wgrad_skinny_bf16", SKINNY_T, M, Nw, D, P(wide), P(narrow), VP(out), transposed, P(ws))

    run_case(be, tag, M, Nw, D, launch, ws_n, S, transposed=transposed, todo=todo, seed=2 * D + transposed)


@pytest.mark.parametrize("backend,D,M", _params([(D, M) for D in SKINNY_D for M in SKINNY_M]))
def test_skinny(backend, be, D, M):
    for tr in (0, 1):
        skinny_case(be, M, 128, D, tr, f"skinny D{D} M{M} tr{tr}", want_S=(M + 31) // 32, todo=plan(be, floats=M in EMU_FLOAT_M))


@pytest.mark.parametrize("backend,D", _params([96, 256]))
def test_skinny_odd_blocks(backend, be, D):
    for M in (33, 289):
        for tr in (0, 1):
            skinny_case(be, M, 384, D, tr, f"skinny Nw384 D{D} M{M} tr{tr}", want_S=(M + 31) // 32, todo=plan(be, floats=M == 33))


@pytest.mark.parametrize("backend,Nw,D,M,S", _params([(32896, 256, 32, 1), (8192, 96, 613, 8)]))
def test_skinny_splits(backend, be, Nw, D, M, S):
    """splits() where its quotient is not the step count: clamped up to 1, and below the steps (slices of 2 and 3 steps, ragged end).  On the
    emulator (8 s and 14 s a call) the exact oracle, one call and one orientation each; the GPU runs everything in both orientations."""
    for tr in ((0, 1) if be.name == "hip" else (int(D == 96),)):
        skinny_case(be, M, Nw, D, tr, f"skinny Nw{Nw} D{D} M{M} tr{tr}", want_S=S, todo=plan(be, floats=False, twice=False))


@pytest.mark.parametrize("backend,D,half_s", _params([(D, h) for D in SKINNY_D for h in (2, 5, 9)], HIP_ONLY))
def test_skinny_multistep(backend, be, D, half_s):
    """Slices of several steps through the product's own splits(): steps = s + 1, 2.5 s (ragged last step), 4.5 s."""
    s = 16 if D == 256 else 32
    steps = s + 1 if half_s == 2 else half_s * s // 2
    M = 32 * steps - (13 if half_s == 5 else 0)
    for tr in (0, 1):
        skinny_case(be, M, 2048, D, tr, f"skinny Nw2048 D{D} M{M} tr{tr}", want_S=s)


@pytest.mark.parametrize("D", SKINNY_D)
@pytest.mark.parametrize("steps,S", SLICES)
def test_skinny_slices(emu_lib, request, steps, S, D):
    """emu_wgrad_skinny_slices: the product's launch<ND> and reduce_kernel with a caller-chosen S, so that a slice has several steps at a
    size the emulator walks in a fraction of a second."""
    be = Backend(request, "emu")
    f = emu_lib.emu_wgrad_skinny_slices
    f.argtypes, f.restype = [L, I, I, I, VP, VP, VP, VP, I], I
    Nw = 128
    for tr, M in enumerate((32 * steps, 32 * steps - 31)):          # the orientation only reaches reduce_kernel: one each
        def launch(wide, narrow, out, ws):
            return f(M, Nw, D, S, P(wide), P(narrow), P(ws), VP(out), tr)
        run_case(be, f"slices D{D} steps{steps} S{S} M{M} tr{tr}", M, Nw, D, launch, S * Nw * D, S, transposed=tr,
                 todo=plan(be, floats=S == 3, twice=tr == 1), seed=2 * D + tr)


# ------------------------------------------------------------------------------------------------ big
def big_splits(M, N1, N2):
    """The slice count the header documents: ceil(256 / tiles) capped to 8 and to the number of stages."""
    tiles = (N1 // 256) * (N2 // 256)
    return max(1, min(-(-256 // tiles), 8, M // 32))


def big_case(be, M, N1, N2, todo):
    tag = f"big {N1}x{N2} M{M}"
    ws_n = size_of(be, "vrwkv_wgrad_big_ws_floats", M, N1, N2)
    S = big_splits(M, N1, N2)
    assert ws_n == (S * N1 * N2 if S > 1 else 0), (tag, ws_n, S)

    def launch(A, B, out, ws):
        return rc_of(be, "vrwkv_wgrad_big_bf16", BIG_T, M, N1, N2, P(A), P(B), VP(out), P(ws))

    run_case(be, tag, M, N1, N2, launch, ws_n, S, todo=todo, seed=1)


@pytest.mark.parametrize("backend,m32", _params(list(BIG_STAGES_M32)))
def test_big_stages(backend, be, m32):
    big_case(be, 32 * m32, 256, 256, plan(be, floats=m32 in (1, 8, 20), twice=m32 <= 12))


@pytest.mark.parametrize("backend,N1,N2,m32", _params([(n1, n2, m) for n1, n2 in BIG_TILES for m in (8, 20)]))
def test_big_tiles(backend, be, N1, N2, m32):
    big_case(be, 32 * m32, N1, N2, plan(be, floats=m32 == 8, twice=False))


@pytest.mark.parametrize("backend", _params([()]))
def test_big_reduce_cap(backend, be):
    """132 tiles, two slices, and a reduce grid of 8448 workgroups capped to 8192.  13 s a call on the emulator: one call with the exact oracle there."""
    big_case(be, 64, 3072, 2816, plan(be, floats=False, twice=False))


@pytest.mark.parametrize("backend,N1,N2,M", _params(list(BIG_LARGE), HIP_ONLY))
def test_big_large(backend, be, N1, N2, M):
    big_case(be, M, N1, N2, plan(be))


# ------------------------------------------------------------------------------------------------ rejections
def _nan(be, n, dtype=torch.bfloat16):
    return torch.full((n,), NAN, dtype=dtype, device=be.dev)


def _untouched(*bufs):
    for b in bufs:
        assert bool(torch.isnan(b.float()).all()), "a rejected call wrote to an output"


@pytest.mark.parametrize("backend", _params([()]))
def test_rejects_skinny(backend, be):
    g = be.gen(11)
    M, Nw, D = 40, 256, 256
    wide, narrow = operand(be, g, "float", M, Nw, 0.5), operand(be, g, "float", M, D, 0.3)
    out, ws = _nan(be, Nw * D + GUARD), _nan(be, 2 * Nw * D + GUARD, torch.float32)
    w, n, o, s = (t.data_ptr() for t in (wide, narrow, out, ws))

    def go(M=M, Nw=Nw, D=D, wide=w, narrow=n, out=o, ws=s):
        return rc_of(be, "vrwkv_wgrad_skinny_bf16", SKINNY_T, M, Nw, D, VP(wide), VP(narrow), VP(out), 0, VP(ws))

    def size(M=M, Nw=Nw, D=D):
        return size_of(be, "vrwkv_wgrad_skinny_ws_floats", M, Nw, D)

    assert go(M=0) == EINVAL and go(M=-32) == EINVAL
    assert go(wide=None) == EINVAL and go(narrow=None) == EINVAL and go(out=None) == EINVAL and go(ws=None) == EINVAL
    assert size(M=0) == -1
    for bad in (dict(Nw=192), dict(Nw=200), dict(Nw=0), dict(D=16), dict(D=48), dict(D=192), dict(D=224)):
        assert go(**bad) == ESHAPE, bad
        assert size(**bad) == -1, bad
    assert go(wide=w + 8) == EALIGN and go(narrow=n + 8) == EALIGN and go(ws=s + 8) == EALIGN
    _untouched(out, ws)
    assert size() == 2 * Nw * D
    assert go() == 0                            # the same arguments without the fault are accepted
    assert bool(torch.isfinite(out[:Nw * D].float()).all())
    _untouched(out[Nw * D:], ws[2 * Nw * D:])


@pytest.mark.parametrize("backend", _params([()]))
def test_rejects_big(backend, be):
    g = be.gen(12)
    M, N1, N2 = 64, 256, 256
    A, B = operand(be, g, "float", M, N1, 0.3), operand(be, g, "float", M, N2, 0.5)
    out, ws = _nan(be, N1 * N2 + GUARD), _nan(be, 2 * N1 * N2 + GUARD, torch.float32)
    a, b, o, s = (t.data_ptr() for t in (A, B, out, ws))

    def go(M=M, N1=N1, N2=N2, A=a, B=b, out=o, ws=s):
        return rc_of(be, "vrwkv_wgrad_big_bf16", BIG_T, M, N1, N2, VP(A), VP(B), VP(out), VP(ws))

    def size(M=M, N1=N1, N2=N2):
        return size_of(be, "vrwkv_wgrad_big_ws_floats", M, N1, N2)

    assert go(M=0) == EINVAL and go(A=None) == EINVAL and go(B=None) == EINVAL and go(out=None) == EINVAL
    assert size(M=0) == -1
    for bad in (dict(M=48), dict(M=63), dict(N1=128), dict(N1=384), dict(N1=0), dict(N2=128), dict(N2=264), dict(N2=0)):
        assert go(**bad) == ESHAPE, bad
        assert size(**bad) == -1, bad
    assert go(A=a + 8) == EALIGN and go(B=b + 8) == EALIGN and go(out=o + 8) == EALIGN and go(ws=s + 8) == EALIGN
    assert size() == 2 * N1 * N2
    assert go(ws=None) == EINVAL                # two slices need their scratch
    _untouched(out, ws)
    # one stage, one slice: no scratch is needed, and none is touched when it is given
    A1, B1 = operand(be, g, "exact", 32, N1, 0), operand(be, g, "exact", 32, N2, 0)
    assert size(M=32) == 0
    assert go(M=32, A=A1.data_ptr(), B=B1.data_ptr(), ws=None) == 0
    want = (A1[:32].double().t() @ B1[:32].double()).float().bfloat16().float()
    assert bool((out[:N1 * N2].view(N1, N2).float() == want).all())
    _untouched(out[N1 * N2:], ws)
    assert go() == 0                            # the same arguments without the fault are accepted
    assert bool(torch.isfinite(out[:N1 * N2].float()).all())
    _untouched(out[N1 * N2:], ws[2 * N1 * N2:])
