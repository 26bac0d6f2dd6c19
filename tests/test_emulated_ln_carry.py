"""The token-shift kernels for one segment of a longer row (vrwkv_ln_mix_fwd_carry_bf16, vrwkv_ln_mix_bwd_carry_bf16, vrwkv_mix_bwd_ln_carry_bf16)
on the host lockstep emulator.  A (B, T) batch is cut along T into pieces; the pieces are chained forward through y_last -> y_prev (the
LayerNorm output of the last row before a cut) and backward, last piece first, through dy_prev -> dy_last (fp32).  Every output, the
statistics and dx are held bit for bit to the uncut launch; parameter gradients (sums over all rows in another grouping) and the gradient
of a non-zero y_prev to 6e-3 rel-RMS against fp64 autograd, the bound of tests/test_emulated_ln.py:94-95 and of the packed test.
Shapes: tests/test_emulated_ln_packed.py::CASES; the cuts fall on the start of a workgroup's range of the uncut launch, inside a range, and
after a single row."""
import ctypes

import pytest
import torch

from tests.test_emulated_ln import P, PA, _inputs, _ln_ref
from tests.test_emulated_ln_packed import CASES

EPS = 1e-5
# cut positions along T per case of CASES (B, T, C, workgroups, _)
CUTS = [
    [[8], [3, 13], [1]],           # (2, 16, 128, 4): ranges of 8 rows -- a cut at a range start, two inside ranges, one after a single row
    [[1, 21], [7]],                # (1, 33, 192, 5): after one row and inside ranges; inactive lanes
    [[2], [1, 4]],                 # (3, 5, 64, 15): one row per workgroup
    [[6], [1]],                    # (2, 12, 128, 1): everything in one range
]
PARAMS = [(*case[:4], cuts) for case, cs in zip(CASES, CUTS) for cuts in cs]
rel = lambda a, r: float((a.double() - r).norm() / r.norm())


def _pieces(T, cuts):
    b = [0, *cuts, T]
    return list(zip(b[:-1], b[1:]))


def _cut(t, B, T, lo, hi):
    """Rows lo..hi-1 of every sample of a (B*T, ...) tensor, as a contiguous (B*(hi-lo), ...) tensor."""
    return t.view(B, T, *t.shape[1:])[:, lo:hi].reshape(B * (hi - lo), *t.shape[1:]).contiguous()


def _put(dst, src, B, T, lo, hi):
    dst.view(B, T, *dst.shape[1:])[:, lo:hi] = src.view(B, hi - lo, *src.shape[1:])


def _fwd(emu, B, T, C, M, x, d, w, b, mus, grid, y_prev=None, want_last=False, carry=True):
    ntok = B * T
    xn = torch.zeros_like(x)
    outs = [torch.zeros_like(x) for _ in range(M)]
    mean, rstd = torch.zeros(ntok), torch.zeros(ntok)
    y_last = torch.zeros(B, C, dtype=torch.bfloat16) if want_last else None
    if carry:
        f = emu.emu_ln_mix_fwd_carry
        f.argtypes = [ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int] + [ctypes.c_void_p] * 11 + [ctypes.c_int]
        assert f(ntok, T, C, EPS, M, P(x), P(d), P(w), P(b), PA(mus), P(xn), PA(outs), P(mean), P(rstd), P(y_prev), P(y_last), grid) == 0
    else:
        f = emu.emu_ln_mix_fwd
        f.argtypes = [ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int] + [ctypes.c_void_p] * 9 + [ctypes.c_int]
        assert f(ntok, T, C, EPS, M, P(x), P(d), P(w), P(b), PA(mus), P(xn), PA(outs), P(mean), P(rstd), grid) == 0
    return xn, outs, mean, rstd, y_last


@pytest.mark.parametrize("M", [1, 6])
@pytest.mark.parametrize("B,T,C,grid,cuts", PARAMS)
def test_forward_pieces_equal_the_uncut_launch(emu_lib, B, T, C, grid, cuts, M):
    x, d, w, b, mus = _inputs(B, T, C, M, seed=B * 100 + T + C + M)
    whole = _fwd(emu_lib, B, T, C, M, x, d, w, b, mus, grid, carry=False)
    # every carry pointer NULL: the existing kernel, bit for bit
    null = _fwd(emu_lib, B, T, C, M, x, d, w, b, mus, grid)
    assert torch.equal(null[0], whole[0]) and torch.equal(null[2], whole[2]) and torch.equal(null[3], whole[3])
    assert all(torch.equal(a_, b_) for a_, b_ in zip(null[1], whole[1]))
    y_prev = None
    for i, (lo, hi) in enumerate(_pieces(T, cuts)):
        n = hi - lo
        g = max(1, min(grid, B * n) - (i % 2))                      # the pieces' own ranges differ from the uncut launch's
        xn, outs, mean, rstd, y_last = _fwd(emu_lib, B, n, C, M, _cut(x, B, T, lo, hi), _cut(d, B, T, lo, hi), w, b, mus, g, y_prev, True)
        assert torch.equal(xn, _cut(whole[0], B, T, lo, hi)), (lo, hi)
        assert torch.equal(mean, _cut(whole[2], B, T, lo, hi)) and torch.equal(rstd, _cut(whole[3], B, T, lo, hi)), (lo, hi)
        for o, ow in zip(outs, whole[1]):
            assert torch.equal(o, _cut(ow, B, T, lo, hi)), (lo, hi)
        y_prev = y_last
    # the last piece's y_last is the LayerNorm output of every sample's last row (up to a statistic's ulp against the torch statement)
    y_r = _ln_ref(x, d, w, b, EPS)[1].view(B, T, C)[:, -1]
    assert float((y_last.float() != y_r.float()).float().mean()) < 0.02


def _autograd(xn_r, w, b, mus, douts, dres, y_prev, dy_last, B, T, C):
    """fp64 autograd from the rounded xn: LayerNorm -> shift that starts from y_prev -> lerps, plus <y[:, -1], dy_last>."""
    xv = xn_r.double().requires_grad_(True)
    wv, bv = w.double().requires_grad_(True), b.double().requires_grad_(True)
    mv = [m.double().requires_grad_(True) for m in mus]
    yp = y_prev.double().requires_grad_(True)
    y = torch.nn.functional.layer_norm(xv, (C,), wv, bv, EPS).view(B, T, C)
    prev = torch.cat([yp.unsqueeze(1), y[:, :-1]], dim=1)
    loss = sum(((y + (prev - y) * m) * do.double().view(B, T, C)).sum() for m, do in zip(mv, douts)) + (y[:, -1] * dy_last.double()).sum()
    loss.backward()
    return xv.grad + (dres.double() if dres is not None else 0), wv.grad, bv.grad, [m.grad for m in mv], yp.grad


def _carries(B, C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, C, generator=g).bfloat16(), torch.randn(B, C, generator=g)          # y_prev (bf16), dy_last (fp32)


@pytest.mark.parametrize("B,T,C,grid,cuts", PARAMS)
def test_channel_mix_backward(emu_lib, B, T, C, grid, cuts):
    x, d, w, b, mus = _inputs(B, T, C, 1, seed=B * 10 + T + C)
    ntok = B * T
    g = torch.Generator().manual_seed(5)
    dout = torch.randn(ntok, C, generator=g).bfloat16()
    dres = torch.randn(ntok, C, generator=g).bfloat16()
    xn_r, y_r, mu_r, rs_r = _ln_ref(x, d, w, b, EPS)
    y0, dyT = _carries(B, C, 11)
    fc = emu_lib.emu_ln_mix_bwd1_carry
    fc.argtypes = [ctypes.c_long, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 14 + [ctypes.c_int]
    f1 = emu_lib.emu_ln_mix_bwd1
    f1.argtypes = [ctypes.c_long, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 11 + [ctypes.c_int]

    def run(lo, hi, y_prev, dy_last, want_prev, grid_):
        n = hi - lo
        cut = lambda t: _cut(t, B, T, lo, hi)
        dx, dwb, dmu = torch.zeros(B * n, C, dtype=torch.bfloat16), torch.zeros(2 * C), torch.zeros(C)
        dy_prev = torch.zeros(B, C) if want_prev else None
        xn_c, mu_c, rs_c, do_c, dr_c = cut(xn_r), cut(mu_r), cut(rs_r), cut(dout), cut(dres)          # alive until the call returns
        assert fc(B * n, n, C, P(xn_c), P(mu_c), P(rs_c), P(w), P(b), P(mus[0]), P(do_c), P(dr_c), P(y_prev), P(dy_last),
                  P(dy_prev), P(dx), P(dwb), P(dmu), grid_) == 0
        return dx, dwb, dmu, dy_prev
    dx_w, dwb_w, dmu_w, dyp_w = run(0, T, y0, dyT, True, grid)                      # the uncut launch, carries at both ends
    dx, dwb, dmu = torch.zeros_like(x), torch.zeros(2 * C), torch.zeros(C)
    dy_last = dyT
    pieces = _pieces(T, cuts)
    for i in reversed(range(len(pieces))):
        lo, hi = pieces[i]
        y_prev = y0 if i == 0 else y_r.view(B, T, C)[:, lo - 1].contiguous()
        dx1, dwb1, dmu1, dy_last = run(lo, hi, y_prev, dy_last, True, max(1, min(grid, B * (hi - lo)) - (i % 2)))
        _put(dx, dx1, B, T, lo, hi)
        dwb += dwb1
        dmu += dmu1
    assert torch.equal(dx, dx_w)
    assert torch.equal(dy_last, dyp_w)                       # Bv of the first rows: the same fp32 sums
    dx_ref, dw_ref, db_ref, dmu_ref, dyp_ref = _autograd(xn_r, w, b, mus, [dout], dres, y0, dyT, B, T, C)
    assert rel(dx, dx_ref) < 6e-3
    assert rel(dwb[:C], dw_ref) < 6e-3 and rel(dwb[C:], db_ref) < 6e-3 and rel(dmu, dmu_ref[0]) < 6e-3
    assert rel(dwb_w[:C], dw_ref) < 6e-3 and rel(dwb_w[C:], db_ref) < 6e-3 and rel(dmu_w, dmu_ref[0]) < 6e-3
    assert rel(dy_last, dyp_ref) < 6e-3
    # every carry pointer NULL: the existing kernel, bit for bit
    dx0, dwb0, dmu0 = torch.zeros_like(x), torch.zeros(2 * C), torch.zeros(C)
    assert f1(ntok, T, C, P(xn_r), P(mu_r), P(rs_r), P(w), P(b), P(mus[0]), P(dout), P(dres), P(dx0), P(dwb0), P(dmu0), grid) == 0
    got = run(0, T, None, None, False, grid)
    assert torch.equal(got[0], dx0) and torch.equal(got[1], dwb0) and torch.equal(got[2], dmu0)


@pytest.mark.parametrize("dup3", [False, True])
@pytest.mark.parametrize("B,T,C,grid,cuts", PARAMS)
def test_time_mix_backward_through_the_c_entry(emu_lib, B, T, C, grid, cuts, dup3):
    """vrwkv_mix_bwd_ln_carry_bf16 (csrc/tmix_fused.hip compiled for the host; it chooses its own grid).  Its dx is the gradient of the
    LayerNorm output, which vrwkv_add_ln_bwd_bf16 takes from there."""
    M = 6
    x, d, w, b, mus = _inputs(B, T, C, M, seed=B * 7 + T + C)
    ntok = B * T
    g = torch.Generator().manual_seed(8)
    douts = [torch.randn(ntok, C, generator=g).bfloat16() for _ in range(M)]
    d3 = torch.randn(ntok, C, generator=g).bfloat16() if dup3 else None
    xn_r, y_r, mu_r, rs_r = _ln_ref(x, d, w, b, EPS)
    y0, dyT = _carries(B, C, 12)
    ws_n = emu_lib.vrwkv_param_grad_ws_floats
    ws_n.restype, ws_n.argtypes = ctypes.c_long, [ctypes.c_long, ctypes.c_int, ctypes.c_int]
    fc = emu_lib.vrwkv_mix_bwd_ln_carry_bf16
    fc.argtypes = [ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 15
    f1 = emu_lib.vrwkv_mix_bwd_ln_bf16
    f1.argtypes = [ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 12

    def run(lo, hi, y_prev, dy_last, want_prev, plain=False):
        n = hi - lo
        cut = lambda t: _cut(t, B, T, lo, hi)
        dx, dmu, ws = torch.zeros(B * n, C, dtype=torch.bfloat16), torch.zeros(M, C), torch.zeros(max(1, ws_n(B * n, C, M)))
        dy_prev = torch.zeros(B, C) if want_prev else None
        do = [cut(t) for t in douts]
        xn_c, mu_c, rs_c, d3_c = cut(xn_r), cut(mu_r), cut(rs_r), cut(d3) if dup3 else None              # alive until the call returns
        args = [P(xn_c), P(mu_c), P(rs_c), P(w), P(b), PA(mus), PA(do), P(d3_c)]
        tail = [P(dx), P(dmu), P(ws), None]
        rc = f1(B * n, n, C, M, *args, *tail) if plain else fc(B * n, n, C, M, *args, P(y_prev), P(dy_last), P(dy_prev), *tail)
        assert rc == 0, rc
        return dx, dmu, dy_prev
    dx_w, dmu_w, dyp_w = run(0, T, y0, dyT, True)
    dx, dmu = torch.zeros_like(x), torch.zeros(M, C)
    dy_last = dyT
    pieces = _pieces(T, cuts)
    for i in reversed(range(len(pieces))):
        lo, hi = pieces[i]
        y_prev = y0 if i == 0 else y_r.view(B, T, C)[:, lo - 1].contiguous()
        dx1, dmu1, dy_last = run(lo, hi, y_prev, dy_last, True)
        _put(dx, dx1, B, T, lo, hi)
        dmu += dmu1
    assert torch.equal(dx, dx_w)
    assert torch.equal(dy_last, dyp_w)
    # fp64 statement from the rounded LayerNorm output
    eff = [(t.double() + d3.double()) if (dup3 and j == 3) else t.double() for j, t in enumerate(douts)]
    y = y_r.double().view(B, T, C)
    prev = torch.cat([y0.double().unsqueeze(1), y[:, :-1]], dim=1)
    bv = sum(e.view(B, T, C) * m.double() for e, m in zip(eff, mus))
    a = sum(e.view(B, T, C) for e in eff) - bv
    dx_ref = a + torch.cat([bv[:, 1:], dyT.double().unsqueeze(1)], dim=1)
    assert rel(dx.view(B, T, C), dx_ref) < 6e-3
    assert rel(dy_last, bv[:, 0]) < 6e-3
    for j in range(M):
        ref = (eff[j].view(B, T, C) * (prev - y)).sum((0, 1))
        assert rel(dmu[j], ref) < 6e-3 and rel(dmu_w[j], ref) < 6e-3, j
    # every carry pointer NULL: the existing entry, bit for bit
    plain = run(0, T, None, None, False, plain=True)
    got = run(0, T, None, None, False)
    assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
