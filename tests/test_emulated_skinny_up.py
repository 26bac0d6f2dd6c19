"""The write-wide LoRA product (csrc/skinny_up.h: w resident as MFMA fragments -- fetched through transposing LDS reads for the (R, C) layout, as it
lies for (C, R) --, lane = token for the streamed narrow tile, the packed output tile through the wave's LDS image and out as row-major 16-byte
pieces) run lane-exactly on the host emulator through its C entry point, against the fp64 product of the bf16 inputs rounded once to bf16."""
import ctypes

import pytest
import torch

VP, L, I = ctypes.c_void_p, ctypes.c_long, ctypes.c_int
GUARD = 0x7FC1                       # a bf16 NaN pattern no product gives: rows past M and the bytes behind out must keep it


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def _operands(M, R, C, cxr, g, integer=False):
    if integer:                      # products and sums of small integers are exact in fp32 in any order
        a = torch.randint(-8, 9, (M, R), generator=g).bfloat16()
        w = torch.randint(-8, 9, (C, R) if cxr else (R, C), generator=g).bfloat16()
    else:
        a = torch.randn(M, R, generator=g).bfloat16()
        w = (torch.randn((C, R) if cxr else (R, C), generator=g) * 0.1).bfloat16()
    ref = a.double() @ (w.double().t() if cxr else w.double())
    return a, w, ref.float().bfloat16().float()           # fp64 -> fp32 is exact enough not to move a bf16 rounding of these sums


def _run(fn, M, R, C, cxr, a, w, *extra):
    tail = 64
    buf = torch.full((M * C + tail,), GUARD, dtype=torch.int16).view(torch.bfloat16)
    rc = fn(M, R, C, *extra, P(a), P(w), int(cxr), P(buf))
    return rc, buf[:M * C].view(M, C), buf[M * C:].view(torch.int16)


def _check(out, tail, want, integer):
    assert bool((tail == GUARD).all()), "bytes behind out were written"
    got = out.float()
    assert not bool(torch.isnan(got).any()), "an element of out was not written"
    if integer:
        assert bool((got == want).all()), f"{int((got != want).sum())} elements differ from the exact product"
    else:                             # one bf16 ulp of the fp64-rounded reference
        assert bool(((got - want).abs() <= 2.0 ** -7 * want.abs() + 1e-6).all())
        assert float((got != want).float().mean()) <= 1e-3


# one strip and two strips of 256 columns in full; strips of 128 (C an odd multiple of 128) with one M per rank
CASES = [(M, C, R, cxr) for M in (1, 31, 33) for C in (256, 512) for R in (32, 96, 256) for cxr in (0, 1)]
CASES += [(M, C, R, cxr) for C in (128, 384) for R, M in ((32, 33), (96, 31), (256, 1)) for cxr in (0, 1)]


@pytest.mark.parametrize("M,C,R,cxr", CASES)
def test_skinny_up_entry(emu_lib, M, C, R, cxr):
    fn = emu_lib.vrwkv_skinny_up_bf16
    fn.argtypes, fn.restype = [L, I, I, VP, VP, I, VP, VP], I
    g = torch.Generator().manual_seed(1000 * M + R + C + cxr)
    for integer in (False, True):
        a, w, want = _operands(M, R, C, cxr, g, integer)
        rc, out, tail = _run(lambda M, R, C, pa, pw, x, po: fn(M, R, C, pa, pw, x, po, None), M, R, C, cxr, a, w)
        assert rc == 0
        _check(out, tail, want, integer)


@pytest.mark.parametrize("M,R,C,cxr", [(257 + 32 * 8, 64, 256, 0), (300, 160, 384, 1), (8 * 32 * 3 + 5, 128, 512, 0), (8 * 32 * 2 + 33, 256, 256, 1),
                                       (8 * 32 + 70, 256, 128, 0)])
def test_skinny_up_walks_several_tiles(emu_lib, M, R, C, cxr):
    """Eight row groups: a workgroup walks 2-4 row tiles, so the narrow tile loaded one tile ahead and the reused LDS image are on the path, and
    the groups do not all have the same number of tiles."""
    fn = emu_lib.emu_skinny_up_groups
    fn.argtypes, fn.restype = [L, I, I, I, VP, VP, I, VP], I
    g = torch.Generator().manual_seed(M + R)
    a, w, want = _operands(M, R, C, cxr, g, integer=True)
    rc, out, tail = _run(fn, M, R, C, cxr, a, w, 8)
    assert rc == 0
    _check(out, tail, want, True)


def test_skinny_up_entry_refuses_in_order(emu_lib):
    fn = emu_lib.vrwkv_skinny_up_bf16
    fn.argtypes, fn.restype = [L, I, I, VP, VP, I, VP, VP], I
    a = torch.zeros(32, 64, dtype=torch.bfloat16)
    w = torch.zeros(64, 128, dtype=torch.bfloat16)
    out = torch.full((32 * 128,), GUARD, dtype=torch.int16)
    EINVAL, ESHAPE = -1, -2
    assert fn(32, 48, 128, None, P(w), 0, P(out), None) == EINVAL          # NULL before the bad rank
    assert fn(32, 64, 128, P(a), None, 0, P(out), None) == EINVAL
    assert fn(32, 64, 128, P(a), P(w), 0, None, None) == EINVAL
    assert fn(0, 48, 128, P(a), P(w), 0, P(out), None) == EINVAL           # M = 0 before the bad rank
    assert fn(32, 48, 128, P(a), P(w), 0, P(out), None) == ESHAPE
    assert fn(32, 64, 192, P(a), P(w), 0, P(out), None) == ESHAPE
    assert bool((out == GUARD).all())
