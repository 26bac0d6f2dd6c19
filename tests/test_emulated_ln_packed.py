"""The token-shift kernels with sample boundaries inside the rows (vrwkv_ln_mix_fwd_packed_bf16, vrwkv_ln_mix_bwd_packed_bf16,
vrwkv_mix_bwd_ln_packed_bf16) on the host lockstep emulator.  `first[n] != 0` marks the first token of a sample: its shifted value is zero and
no gradient goes from it to the row before.  Outputs and dx are held bit for bit to the EXISTING kernels run on every segment alone; the
parameter gradients (sums over all rows in another grouping) to 6e-3 rel-RMS against fp64 autograd, the bound of tests/test_emulated_ln.py:94-95."""
import ctypes

import pytest
import torch

from tests.test_emulated_ln import P, PA, _inputs, _ln_ref

EPS = 1e-5
# (B, T, C, workgroups, segment lengths per row): resets at rows that are and are not the start of a workgroup's range
CASES = [
    (2, 16, 128, 4, [[8, 8], [3, 13]]),           # ranges of 8 rows: a reset at a range start (row 8, row 24) and inside one (row 19)
    (1, 33, 192, 5, [[1, 20, 12]]),                # a one-token sample; inactive lanes (C / 8 = 24)
    (3, 5, 64, 15, [[5], [2, 3], [4, 1]]),         # one row per workgroup
    (2, 12, 128, 1, [[6, 6], [12]]),               # everything in one range
]


def _first(B, T, segs):
    f = torch.zeros(B, T, dtype=torch.uint8)
    bounds = []
    for b, row in enumerate(segs):
        assert sum(row) == T
        t = 0
        for n in row:
            f[b, t] = 1
            bounds.append((b * T + t, b * T + t + n))
            t += n
    return f.view(-1).contiguous(), bounds


def _fwd(emu, ntok, T, C, M, x, d, w, b, mus, grid, first=None, packed=False):
    xn = torch.zeros_like(x)
    outs = [torch.zeros_like(x) for _ in range(M)]
    mean, rstd = torch.zeros(ntok), torch.zeros(ntok)
    if packed:
        f = emu.emu_ln_mix_fwd_packed
        f.argtypes = [ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int] + [ctypes.c_void_p] * 10 + [ctypes.c_int]
        assert f(ntok, T, C, EPS, M, P(x), P(d), P(w), P(b), PA(mus), P(xn), PA(outs), P(mean), P(rstd), P(first), grid) == 0
    else:
        f = emu.emu_ln_mix_fwd
        f.argtypes = [ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int] + [ctypes.c_void_p] * 9 + [ctypes.c_int]
        assert f(ntok, T, C, EPS, M, P(x), P(d), P(w), P(b), PA(mus), P(xn), PA(outs), P(mean), P(rstd), grid) == 0
    return xn, outs, mean, rstd


@pytest.mark.parametrize("M", [1, 6])
@pytest.mark.parametrize("B,T,C,grid,segs", CASES)
def test_forward_equals_the_existing_kernel_per_segment(emu_lib, B, T, C, grid, segs, M):
    x, d, w, b, mus = _inputs(B, T, C, M, seed=B * 100 + T + C + M)
    ntok = B * T
    first, bounds = _first(B, T, segs)
    xn, outs, mean, rstd = _fwd(emu_lib, ntok, T, C, M, x, d, w, b, mus, grid, first, packed=True)
    for lo, hi in bounds:
        n = hi - lo
        xs, ds = x[lo:hi].contiguous(), d[lo:hi].contiguous()
        xn1, outs1, mean1, rstd1 = _fwd(emu_lib, n, n, C, M, xs, ds, w, b, mus, 1)
        assert torch.equal(xn[lo:hi], xn1) and torch.equal(mean[lo:hi], mean1) and torch.equal(rstd[lo:hi], rstd1), (lo, hi)
        for o, o1 in zip(outs, outs1):
            assert torch.equal(o[lo:hi], o1), (lo, hi)
    # no flag set / flags only where n % T == 0 already says so: the existing kernel, bit for bit
    plain = _fwd(emu_lib, ntok, T, C, M, x, d, w, b, mus, grid)
    none = _fwd(emu_lib, ntok, T, C, M, x, d, w, b, mus, grid, torch.zeros(ntok, dtype=torch.uint8), packed=True)
    rows = _fwd(emu_lib, ntok, T, C, M, x, d, w, b, mus, grid, _first(B, T, [[T]] * B)[0], packed=True)
    for got in (none, rows):
        assert torch.equal(got[0], plain[0]) and torch.equal(got[2], plain[2]) and torch.equal(got[3], plain[3])
        assert all(torch.equal(a_, b_) for a_, b_ in zip(got[1], plain[1]))


def _autograd(xn_r, w, b, mus, douts, first, dres, B, T, C):
    """fp64 autograd from the rounded xn: LayerNorm -> masked shift -> lerps; returns dx, dgamma, dbeta, [dmu_j]."""
    xv = xn_r.double().requires_grad_(True)
    wv, bv = w.double().requires_grad_(True), b.double().requires_grad_(True)
    mv = [m.double().requires_grad_(True) for m in mus]
    y = torch.nn.functional.layer_norm(xv, (C,), wv, bv, EPS)
    prev = torch.cat([torch.zeros_like(y[:1]), y[:-1]], dim=0).masked_fill(first.view(-1, 1).bool(), 0)
    loss = sum(((y + (prev - y) * m) * do.double()).sum() for m, do in zip(mv, douts))
    loss.backward()
    return xv.grad + (dres.double() if dres is not None else 0), wv.grad, bv.grad, [m.grad for m in mv]


rel = lambda a, r: float((a.double() - r).norm() / r.norm())


@pytest.mark.parametrize("B,T,C,grid,segs", CASES)
def test_channel_mix_backward(emu_lib, B, T, C, grid, segs):
    x, d, w, b, mus = _inputs(B, T, C, 1, seed=B * 10 + T + C)
    ntok = B * T
    first, bounds = _first(B, T, segs)
    g = torch.Generator().manual_seed(5)
    dout = torch.randn(ntok, C, generator=g).bfloat16()
    dres = torch.randn(ntok, C, generator=g).bfloat16()
    xn_r, y_r, mu_r, rs_r = _ln_ref(x, d, w, b, EPS)
    fp = emu_lib.emu_ln_mix_bwd1_packed
    fp.argtypes = [ctypes.c_long, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 12 + [ctypes.c_int]
    f1 = emu_lib.emu_ln_mix_bwd1
    f1.argtypes = [ctypes.c_long, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 11 + [ctypes.c_int]

    def packed(flags):
        dx, dwb, dmu = torch.zeros_like(x), torch.zeros(2 * C), torch.zeros(C)
        assert fp(ntok, T, C, P(xn_r), P(mu_r), P(rs_r), P(w), P(b), P(mus[0]), P(dout), P(dres), P(flags), P(dx), P(dwb), P(dmu), grid) == 0
        return dx, dwb, dmu
    dx, dwb, dmu = packed(first)
    for lo, hi in bounds:                                   # dx: the existing kernel on the segment alone
        n = hi - lo
        dx1, dwb1, dmu1 = torch.zeros(n, C, dtype=torch.bfloat16), torch.zeros(2 * C), torch.zeros(C)
        assert f1(n, n, C, P(xn_r[lo:hi].contiguous()), P(mu_r[lo:hi].contiguous()), P(rs_r[lo:hi].contiguous()), P(w), P(b), P(mus[0]),
                  P(dout[lo:hi].contiguous()), P(dres[lo:hi].contiguous()), P(dx1), P(dwb1), P(dmu1), 1) == 0
        assert torch.equal(dx[lo:hi], dx1), (lo, hi)
    dx_ref, dw_ref, db_ref, dmu_ref = _autograd(xn_r, w, b, mus, [dout], first, dres, B, T, C)
    assert rel(dx, dx_ref) < 6e-3
    assert rel(dwb[:C], dw_ref) < 6e-3 and rel(dwb[C:], db_ref) < 6e-3 and rel(dmu, dmu_ref[0]) < 6e-3
    # flags that say nothing new: the existing kernel, bit for bit
    dx0, dwb0, dmu0 = torch.zeros_like(x), torch.zeros(2 * C), torch.zeros(C)
    assert f1(ntok, T, C, P(xn_r), P(mu_r), P(rs_r), P(w), P(b), P(mus[0]), P(dout), P(dres), P(dx0), P(dwb0), P(dmu0), grid) == 0
    for got in (packed(torch.zeros(ntok, dtype=torch.uint8)), packed(_first(B, T, [[T]] * B)[0])):
        assert torch.equal(got[0], dx0) and torch.equal(got[1], dwb0) and torch.equal(got[2], dmu0)


@pytest.mark.parametrize("dup3", [False, True])
@pytest.mark.parametrize("B,T,C,grid,segs", CASES[:3])
def test_time_mix_backward_through_the_c_entry(emu_lib, B, T, C, grid, segs, dup3):
    """vrwkv_mix_bwd_ln_packed_bf16 (csrc/tmix_fused.hip compiled for the host; it chooses its own grid)."""
    M = 6
    x, d, w, b, mus = _inputs(B, T, C, M, seed=B * 7 + T + C)
    ntok = B * T
    first, bounds = _first(B, T, segs)
    g = torch.Generator().manual_seed(8)
    douts = [torch.randn(ntok, C, generator=g).bfloat16() for _ in range(M)]
    d3 = torch.randn(ntok, C, generator=g).bfloat16() if dup3 else None
    xn_r, y_r, mu_r, rs_r = _ln_ref(x, d, w, b, EPS)
    ws_n = emu_lib.vrwkv_param_grad_ws_floats
    ws_n.restype, ws_n.argtypes = ctypes.c_long, [ctypes.c_long, ctypes.c_int, ctypes.c_int]
    fp = emu_lib.vrwkv_mix_bwd_ln_packed_bf16
    fp.argtypes = [ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 13
    f1 = emu_lib.vrwkv_mix_bwd_ln_bf16
    f1.argtypes = [ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 12

    def run(n, Tn, sl, flags, packed):
        cut = lambda t: t[sl].contiguous()
        dx, dmu, ws = torch.zeros(n, C, dtype=torch.bfloat16), torch.zeros(M, C), torch.zeros(max(1, ws_n(n, C, M)))
        do = [cut(t) for t in douts]
        args = [P(cut(xn_r)), P(cut(mu_r)), P(cut(rs_r)), P(w), P(b), PA(mus), PA(do), P(cut(d3)) if dup3 else None]
        tail = [P(dx), P(dmu), P(ws), None]
        rc = fp(n, Tn, C, M, *args, P(flags), *tail) if packed else f1(n, Tn, C, M, *args, *tail)
        assert rc == 0, rc
        return dx, dmu
    dx, dmu = run(ntok, T, slice(0, ntok), first, True)
    for lo, hi in bounds:
        dx1, _ = run(hi - lo, hi - lo, slice(lo, hi), None, False)
        assert torch.equal(dx[lo:hi], dx1), (lo, hi)
    eff = [t if not (dup3 and j == 3) else (t.float() + d3.float()) for j, t in enumerate(douts)]
    xv = xn_r.double()
    y = torch.nn.functional.layer_norm(xv, (C,), w.double(), b.double(), EPS).float().bfloat16().double()     # the rounded LayerNorm output
    prev = torch.cat([torch.zeros_like(y[:1]), y[:-1]], dim=0).masked_fill(first.view(-1, 1).bool(), 0)
    for j in range(M):
        ref = (eff[j].double() * (prev - y)).sum(0)
        assert rel(dmu[j], ref) < 6e-3, j
    plain = run(ntok, T, slice(0, ntok), None, False)
    for flags in (None, torch.zeros(ntok, dtype=torch.uint8), _first(B, T, [[T]] * B)[0]):
        got = run(ntok, T, slice(0, ntok), flags, True)
        assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
