"""csrc/skinny_up.h on the MI355X: the write-wide LoRA product out (M, C) = a (M, R) . w for both layouts of w, through the C entry point and
through fused._LoraMM.

Reference of the entry tests: the fp64 product of the bf16 inputs, rounded once to bf16.  Pass criterion: every element within one bf16 ulp of it,
|got - ref| <= 2^-7 |ref| + 1e-6, and at most 1e-3 of the elements different at all (an fp32-accumulated product of a ~ N(0, 1), w ~ N(0, 0.1^2)
differs from that reference in <= 1e-4 of the elements, always by one ulp, in plain and in 16-wide chunked summation order: the cap leaves 10x)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

RANKS = (32, 64, 96, 128, 160, 256)
MS = (1, 31, 32, 33, 257)
CS = (256, 768, 2048, 128, 384)       # one strip of 256 columns, three, eight; strips of 128 where C is an odd multiple of 128: one and three
GUARD = 0x7FC1                        # a bf16 NaN pattern no product gives
TAIL = 4096


def _lib():
    from visualrwkv_amd import hip_lib
    return hip_lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def operands():
    """a (257, R) ~ N(0, 1) and w ~ N(0, 0.1^2) in both layouts for every rank at the widest C, made once; the cases slice them (rows of a, rows or
    columns of w -- sliced copies are contiguous), and the fp64 references are products of those slices."""
    g = torch.Generator(device="cuda").manual_seed(20)
    ops = {}
    for R in RANKS:
        a = torch.randn(max(MS), R, device="cuda", generator=g).bfloat16()
        w_rc = (torch.randn(R, max(CS), device="cuda", generator=g) * 0.1).bfloat16()
        w_cr = (torch.randn(max(CS), R, device="cuda", generator=g) * 0.1).bfloat16()
        ops[R] = (a, w_rc, w_cr)
    return ops


@pytest.mark.parametrize("cxr", [0, 1])
@pytest.mark.parametrize("R", RANKS)
def test_entry_matches_fp64_product_and_keeps_its_bounds(operands, R, cxr):
    lib = _lib()
    a_all, w_rc, w_cr = operands[R]
    ndiff = ntotal = 0
    for C in CS:
        w = (w_cr[:C] if cxr else w_rc[:, :C]).contiguous()
        ref_all = (a_all.double() @ (w.double().t() if cxr else w.double())).float().bfloat16().float()
        for M in MS:
            a = a_all[:M].contiguous()
            rows = (M + 31) // 32 * 32                     # the rows after a ragged M belong to the guard too
            buf = torch.full((rows * C + TAIL,), GUARD, dtype=torch.int16, device="cuda")
            rc = lib.vrwkv_skinny_up_bf16(M, R, C, a.data_ptr(), w.data_ptr(), cxr, buf.data_ptr(), _stream())
            assert rc == 0, (M, C, rc)
            torch.cuda.synchronize()
            assert bool((buf[M * C:] == GUARD).all()), f"M={M} C={C}: rows past M or bytes behind out were written"
            got, ref = buf[:M * C].view(torch.bfloat16).view(M, C).float(), ref_all[:M]
            assert not bool(torch.isnan(got).any()), f"M={M} C={C}: an element was not written"
            err = (got - ref).abs()
            bad = err > 2.0 ** -7 * ref.abs() + 1e-6
            ndiff_case = int((got != ref).sum())
            ndiff, ntotal = ndiff + ndiff_case, ntotal + M * C
            assert not bool(bad.any()), f"M={M} C={C}: {int(bad.sum())} elements off by more than one bf16 ulp, max {float(err.max())}"
            # The share is a rate: in the M = 1 cases a single element of 128 .. 768 is already 1.3e-3 .. 7.8e-3, and at the 1e-4 a correct kernel gives one
            # of their ~3 600 elements per (R, layout) is expected to differ.  So the cap is applied to every case of at least 8 192 elements (one
            # element there is 1.2e-4) and to all cases of this (R, layout) together, the M = 1 ones included.
            if M * C >= 8192:
                assert ndiff_case <= 1e-3 * M * C, f"M={M} C={C}: {ndiff_case / (M * C)} of the elements differ from the rounded fp64 product"
    print(f"R={R} w_is_CxR={cxr}: {ndiff} of {ntotal} elements differ from the rounded fp64 product ({ndiff / ntotal:.2e})")
    assert ndiff <= 1e-3 * ntotal


def test_entry_refuses_defective_calls_in_order_and_writes_nothing():
    lib = _lib()
    a = torch.zeros(32, 64, dtype=torch.bfloat16, device="cuda")
    w = torch.zeros(64, 256, dtype=torch.bfloat16, device="cuda")
    out = torch.full((32 * 256,), GUARD, dtype=torch.int16, device="cuda")
    EINVAL, ESHAPE = -1, -2
    st = _stream()
    A, W, O = a.data_ptr(), w.data_ptr(), out.data_ptr()
    null = ctypes.c_void_p(0)
    assert lib.vrwkv_skinny_up_bf16(32, 48, 192, null, W, 0, O, st) == EINVAL          # NULL comes before the bad shape
    assert lib.vrwkv_skinny_up_bf16(32, 64, 256, A, null, 0, O, st) == EINVAL
    assert lib.vrwkv_skinny_up_bf16(32, 64, 256, A, W, 0, null, st) == EINVAL
    assert lib.vrwkv_skinny_up_bf16(0, 48, 256, A, W, 0, O, st) == EINVAL              # M = 0 comes before the bad rank
    assert lib.vrwkv_skinny_up_bf16(32, 48, 256, A, W, 0, O, st) == ESHAPE
    assert lib.vrwkv_skinny_up_bf16(32, 64, 192, A, W, 0, O, st) == ESHAPE
    assert lib.vrwkv_skinny_up_bf16(32, 48, 256, A, W, 1, O, st) == ESHAPE
    torch.cuda.synchronize()
    assert bool((out == GUARD).all())


def _lora_mm_case():
    M, C, r = 257, 768, 64
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(M, C, device="cuda", generator=g).bfloat16().requires_grad_()
    h = torch.randn(M, r, device="cuda", generator=g).bfloat16().requires_grad_()
    w1 = (torch.randn(C, r, device="cuda", generator=g) * 0.1).bfloat16().requires_grad_()
    w2 = (torch.randn(r, C, device="cuda", generator=g) * 0.1).bfloat16().requires_grad_()
    dy_up = torch.randn(M, C, device="cuda", generator=g).bfloat16()
    dy_down = torch.randn(M, r, device="cuda", generator=g).bfloat16()
    return (h, w2, dy_up), (x, w1, dy_down)


def _run(mm, inp, w, dy):
    inp.grad = w.grad = None
    y = mm(inp, w)
    y.backward(dy)
    return y.detach(), inp.grad.clone(), w.grad.clone()


def test_lora_mm_with_the_kernel_matches_plain_matmul(monkeypatch):
    """fused.lora_mm at (M, C, r) = (257, 768, 64) against torch.matmul, the up-projection h @ w2 (the kernel writes the output) and the
    down-projection x @ w1 (the kernel writes the input gradient).  tests/test_fused_gpu.py::test_lora_mm_gradients_match_plain_matmul asks two things:
    what the SAME kernel computes on both sides is bit-equal, what another kernel computes (there the skinny weight gradient) is within 1e-2 of the
    largest element.  Here the write-wide product is another kernel on one side, so its results are held to that second bound -- and to the tighter one
    of this module: every element within one bf16 ulp of the library's, two roundings of fp32 sums that differ in their last bits."""
    from visualrwkv_amd import fused
    monkeypatch.setattr(fused, "LORA_UP", True)
    monkeypatch.setattr(fused, "SKINNY_UP_CASES", frozenset({(64, 0), (64, 1)}))
    calls = []
    real = fused.skinny_up
    monkeypatch.setattr(fused, "skinny_up", lambda a, w, l: (calls.append((tuple(a.shape), tuple(w.shape), l)), real(a, w, l))[1])
    up, down = _lora_mm_case()

    def close(u, v, what):
        u, v = u.float(), v.float()
        print(f"{what}: bit-equal {bool(torch.equal(u, v))}, share differing {float((u != v).float().mean()):.2e}, "
              f"max |diff| / max |ref| {float((u - v).abs().max() / v.abs().max()):.2e}")
        assert float((u - v).abs().max() / v.abs().max()) < 1e-2
        assert bool(((u - v).abs() <= 2.0 ** -7 * v.abs() + 1e-6).all())

    y, dh, dw2 = _run(fused.lora_mm, *up)
    yr, dhr, dw2r = _run(torch.matmul, *up)
    assert calls == [((257, 64), (64, 768), 0)]            # the output; dh = dy @ w2^T is read-wide: library
    close(y, yr, "h @ w2")
    assert torch.equal(dh, dhr)
    assert float((dw2.float() - dw2r.float()).abs().max() / dw2r.float().abs().max()) < 1e-2
    del calls[:]
    y, dx, dw1 = _run(fused.lora_mm, *down)
    yr, dxr, dw1r = _run(torch.matmul, *down)
    assert calls == [((257, 64), (768, 64), 1)]            # the input gradient; x @ w1 is read-wide: library
    assert torch.equal(y, yr)
    close(dx, dxr, "dh @ w1^T")
    assert float((dw1.float() - dw1r.float()).abs().max() / dw1r.float().abs().max()) < 1e-2


def test_lora_mm_with_the_switch_off_stays_on_the_library(monkeypatch):
    from visualrwkv_amd import fused
    monkeypatch.setattr(fused, "LORA_UP", False)

    def boom(*a, **k):
        raise AssertionError("csrc/skinny_up.h was called with VRWKV_LORA_UP=0")
    monkeypatch.setattr(fused, "skinny_up", boom)
    for case in _lora_mm_case():
        got, ref = _run(fused.lora_mm, *case), _run(torch.matmul, *case)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


def test_dispatch_takes_only_write_wide_products_of_supported_tensors(monkeypatch):
    from visualrwkv_amd import fused
    monkeypatch.setattr(fused, "LORA_UP", True)
    monkeypatch.setattr(fused, "SKINNY_UP_CASES", frozenset({(64, 0), (64, 1)}))
    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device="cuda")
    assert fused.skinny_up_supported(z(33, 64), z(64, 768), 0) and fused.skinny_up_supported(z(33, 64), z(768, 64), 1)
    assert not fused.skinny_up_supported(z(33, 768), z(768, 64), 0)              # read-wide
    assert not fused.skinny_up_supported(z(33, 768), z(64, 768), 1)
    assert not fused.skinny_up_supported(z(33, 96), z(96, 768), 0)               # a rank the dispatch table does not hold
    assert not fused.skinny_up_supported(z(33, 64), z(64, 192), 0)               # C % 128
    assert not fused.skinny_up_supported(z(33, 128)[:, :64], z(64, 768), 0)      # not contiguous
    assert not fused.skinny_up_supported(z(33, 64).float(), z(64, 768).float(), 0)
    assert not fused.skinny_up_supported(z(33, 64).cpu(), z(64, 768).cpu(), 0)
    assert not fused.skinny_up_supported(z(33, 64), z(64, 768), 1)               # w (64, 768) read as (C, R): the ranks do not match
    assert not fused.skinny_up_supported(z(34 * 64)[4:4 + 33 * 64].view(33, 64), z(64, 768), 0)     # 8 bytes off a 16-byte boundary
