"""The token-shift entries with sample boundaries inside the rows on the MI355X (vrwkv_ln_mix_fwd_packed_bf16, vrwkv_ln_mix_bwd_packed_bf16,
vrwkv_mix_bwd_ln_packed_bf16): outputs and dx bit for bit those of the existing entries run on every segment alone, parameter gradients within
the 6e-3 rel-RMS of tests/test_emulated_ln.py:94-95 of the per-segment sums, and first == NULL / flags that say nothing new = the existing
entry.  The emulator tests (tests/test_emulated_ln_packed.py) hold the same kernels against fp64 autograd."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-5
CASES = [(2, 64, 2048, [[32, 32], [48, 16]]), (3, 208, 1024, [[16, 96, 96], [208], [1, 7, 200]]), (4, 2624, 2048, [[640, 704, 1280], [2624], [800, 1824], [16] * 164])]


def PA(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _p(t):
    return t.data_ptr() if t is not None else None


def _inputs(B, T, C, M, seed):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=g)
    x, d = mk(B * T, C).bfloat16().cuda(), (0.5 * mk(B * T, C)).bfloat16().cuda()
    w, b = (1 + 0.2 * mk(C)).bfloat16().cuda(), (0.1 * mk(C)).bfloat16().cuda()
    mus = [torch.rand(C, generator=g).bfloat16().cuda() for _ in range(M)]
    douts = [mk(B * T, C).bfloat16().cuda() for _ in range(M + 1)]
    return x, d, w, b, mus, douts


def _first(B, T, segs):
    f = torch.zeros(B, T, dtype=torch.uint8)
    bounds = []
    for r, row in enumerate(segs):
        assert sum(row) == T
        t = 0
        for n in row:
            f[r, t] = 1
            bounds.append((r * T + t, r * T + t + n))
            t += n
    return f.view(-1).cuda(), bounds


def _fwd(lib, n, T, C, M, x, d, w, b, mus, first):
    xn, outs = torch.empty_like(x), [torch.empty_like(x) for _ in range(M)]
    mean, rstd = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    if first is False:
        rc = lib.vrwkv_ln_mix_fwd_bf16(n, T, C, EPS, M, x.data_ptr(), d.data_ptr(), w.data_ptr(), b.data_ptr(), PA(mus), xn.data_ptr(), PA(outs),
                                       mean.data_ptr(), rstd.data_ptr(), st)
    else:
        rc = lib.vrwkv_ln_mix_fwd_packed_bf16(n, T, C, EPS, M, x.data_ptr(), d.data_ptr(), w.data_ptr(), b.data_ptr(), PA(mus), xn.data_ptr(), PA(outs),
                                              mean.data_ptr(), rstd.data_ptr(), _p(first), st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return xn, outs, mean, rstd


def _bwd(lib, n, T, C, M, xn, mean, rstd, w, b, mus, douts, dres, second, first):
    """dx (the gradient of xn), parameter gradients; first=False: the existing entries."""
    st = torch.cuda.current_stream().cuda_stream
    dx, dmu = torch.empty_like(xn), torch.empty(M, C, device="cuda")
    if M == 1:
        dwb = torch.empty(2, C, device="cuda")
        ws = torch.empty(lib.vrwkv_ln_mix_ws_floats(n, C, M), device="cuda")
        head = (n, T, C, M, xn.data_ptr(), mean.data_ptr(), rstd.data_ptr(), w.data_ptr(), b.data_ptr(), PA(mus), PA(douts[:M]), None, dres.data_ptr())
        tail = (dx.data_ptr(), dwb.data_ptr(), dmu.data_ptr(), ws.data_ptr(), st)
        rc = lib.vrwkv_ln_mix_bwd_bf16(*head, *tail) if first is False else lib.vrwkv_ln_mix_bwd_packed_bf16(*head, _p(first), *tail)
        out = (dx, dmu, dwb)
    else:
        ws = torch.empty(max(1, lib.vrwkv_param_grad_ws_floats(n, C, M)), device="cuda")
        head = (n, T, C, M, xn.data_ptr(), mean.data_ptr(), rstd.data_ptr(), w.data_ptr(), b.data_ptr(), PA(mus), PA(douts[:M]), _p(second))
        tail = (dx.data_ptr(), dmu.data_ptr(), ws.data_ptr(), st)
        rc = lib.vrwkv_mix_bwd_ln_bf16(*head, *tail) if first is False else lib.vrwkv_mix_bwd_ln_packed_bf16(*head, _p(first), *tail)
        out = (dx, dmu)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out


rel = lambda a, r: float((a.double() - r.double()).norm() / r.double().norm())


@pytest.mark.parametrize("M", [1, 6])
@pytest.mark.parametrize("B,T,C,segs", CASES)
def test_packed_shift_entries(hip_lib, B, T, C, segs, M):
    x, d, w, b, mus, douts = _inputs(B, T, C, M, seed=B + T + C + M)
    n = B * T
    first, bounds = _first(B, T, segs)
    dres, second = douts[M], (douts[M] if M == 6 else None)
    xn, outs, mean, rstd = _fwd(hip_lib, n, T, C, M, x, d, w, b, mus, first)
    got = _bwd(hip_lib, n, T, C, M, xn, mean, rstd, w, b, mus, douts, dres, second, first)
    sums = [torch.zeros_like(t) for t in got[1:]]
    if len(bounds) > 40:                                     # the row of 164 one-chunk samples: every tenth, both ends
        bounds = bounds[:3] + bounds[3:-3:10] + bounds[-3:]
        sums = None
    for lo, hi in bounds:
        m = hi - lo
        cut = lambda t: t[lo:hi].contiguous()
        xn1, outs1, mean1, rstd1 = _fwd(hip_lib, m, m, C, M, cut(x), cut(d), w, b, mus, False)
        assert torch.equal(xn[lo:hi], xn1) and torch.equal(mean[lo:hi], mean1) and torch.equal(rstd[lo:hi], rstd1), (lo, hi)
        assert all(torch.equal(o[lo:hi], o1) for o, o1 in zip(outs, outs1)), (lo, hi)
        one = _bwd(hip_lib, m, m, C, M, xn1, mean1, rstd1, w, b, mus, [cut(t) for t in douts], cut(dres), cut(second) if second is not None else None, False)
        assert torch.equal(got[0][lo:hi], one[0]), (lo, hi)
        if sums is not None:
            for s_, t_ in zip(sums, one[1:]):
                s_ += t_
    if sums is not None:
        for a_, s_ in zip(got[1:], sums):
            assert rel(a_, s_) < 6e-3
    # NULL, all zeros, and flags only where n % T == 0 says so already: the existing entries, bit for bit
    plain_f = _fwd(hip_lib, n, T, C, M, x, d, w, b, mus, False)
    plain_b = _bwd(hip_lib, n, T, C, M, plain_f[0], plain_f[2], plain_f[3], w, b, mus, douts, dres, second, False)
    for flags in (None, torch.zeros(n, dtype=torch.uint8, device="cuda"), _first(B, T, [[T]] * B)[0]):
        f = _fwd(hip_lib, n, T, C, M, x, d, w, b, mus, flags)
        assert torch.equal(f[0], plain_f[0]) and torch.equal(f[2], plain_f[2]) and torch.equal(f[3], plain_f[3])
        assert all(torch.equal(a_, b_) for a_, b_ in zip(f[1], plain_f[1]))
        bb = _bwd(hip_lib, n, T, C, M, f[0], f[2], f[3], w, b, mus, douts, dres, second, flags)
        assert all(torch.equal(a_, b_) for a_, b_ in zip(bb, plain_b))
