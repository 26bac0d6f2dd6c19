"""The token-shift entries for one segment of a longer row on the MI355X (vrwkv_ln_mix_fwd_carry_bf16, vrwkv_ln_mix_bwd_carry_bf16,
vrwkv_mix_bwd_ln_carry_bf16): a (B, T) batch cut along T, the pieces chained forward through y_last -> y_prev and backward, last piece first,
through dy_prev -> dy_last.  Every output, the statistics and dx are bit for bit those of the uncut launch; parameter gradients summed over
the pieces, and the gradient of a non-zero y_prev, within the 6e-3 rel-RMS of tests/test_emulated_ln.py:94-95 of fp64 autograd; every carry
pointer NULL = the existing entry.  tests/test_emulated_ln_carry.py holds the same statements on the emulator.
Last, fused.add_ln_mix -- the autograd Function over the plain, _packed and _carry entries -- against the same drivers at the smallest shape."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-5
# (B, T, C, cut positions along T)
CASES = [(2, 64, 2048, [16]), (2, 64, 2048, [1, 33]), (3, 208, 1024, [16, 112]), (16, 2624, 2048, [1312]), (16, 2624, 2048, [656, 1312, 1968])]


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
    y0, dyT = mk(B, C).bfloat16().cuda(), mk(B, C).cuda()
    return x, d, w, b, mus, douts, y0, dyT


def _cut(t, B, T, lo, hi):
    return t.view(B, T, *t.shape[1:])[:, lo:hi].reshape(B * (hi - lo), *t.shape[1:]).contiguous()


def _fwd(lib, B, T, C, M, x, d, w, b, mus, y_prev=None, want_last=False, plain=False, first=None):
    """d None: no residual add, xn is x itself.  first: the marks of packed rows -- the _packed entry in place of the _carry one."""
    n = B * T
    xn, outs = (torch.empty_like(x) if d is not None else x), [torch.empty_like(x) for _ in range(M)]
    mean, rstd = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    y_last = torch.empty(B, C, dtype=torch.bfloat16, device="cuda") if want_last else None
    st = torch.cuda.current_stream().cuda_stream
    head = (n, T, C, EPS, M, x.data_ptr(), _p(d), w.data_ptr(), b.data_ptr(), PA(mus), xn.data_ptr() if d is not None else None, PA(outs),
            mean.data_ptr(), rstd.data_ptr())
    if first is not None:
        rc = lib.vrwkv_ln_mix_fwd_packed_bf16(*head, first.data_ptr(), st)
    else:
        rc = lib.vrwkv_ln_mix_fwd_bf16(*head, st) if plain else lib.vrwkv_ln_mix_fwd_carry_bf16(*head, _p(y_prev), _p(y_last), st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return xn, outs, mean, rstd, y_last


def _bwd(lib, B, T, C, M, xn, mean, rstd, w, b, mus, douts, dres, second, y_prev=None, dy_last=None, want_prev=False, plain=False, first=None):
    """(dx, dmu, dwb, dy_prev): dx = the gradient of xn (M = 6: the shift's backward, then vrwkv_add_ln_bwd_bf16, as fused._AddLnMix).
    first: the marks of packed rows -- the _packed entries in place of the _carry ones."""
    n = B * T
    st = torch.cuda.current_stream().cuda_stream
    dx, dmu, dwb = torch.empty_like(xn), torch.empty(M, C, device="cuda"), torch.empty(2, C, device="cuda")
    dy_prev = torch.empty(B, C, device="cuda") if want_prev else None
    carry = () if plain else (first.data_ptr(),) if first is not None else (_p(y_prev), _p(dy_last), _p(dy_prev))
    if M == 1:
        ws = torch.empty(lib.vrwkv_ln_mix_ws_floats(n, C, M), device="cuda")
        head = (n, T, C, M, xn.data_ptr(), mean.data_ptr(), rstd.data_ptr(), w.data_ptr(), b.data_ptr(), PA(mus), PA(douts[:M]), None, _p(dres))
        tail = (dx.data_ptr(), dwb.data_ptr(), dmu.data_ptr(), ws.data_ptr(), st)
        entry = lib.vrwkv_ln_mix_bwd_bf16 if plain else lib.vrwkv_ln_mix_bwd_packed_bf16 if first is not None else lib.vrwkv_ln_mix_bwd_carry_bf16
        rc = entry(*head, *carry, *tail)
        assert rc == 0, rc
    else:
        dy = torch.empty_like(xn)
        ws = torch.empty(max(1, lib.vrwkv_param_grad_ws_floats(n, C, M)), device="cuda")
        head = (n, T, C, M, xn.data_ptr(), mean.data_ptr(), rstd.data_ptr(), w.data_ptr(), b.data_ptr(), PA(mus), PA(douts[:M]), _p(second))
        entry = lib.vrwkv_mix_bwd_ln_bf16 if plain else lib.vrwkv_mix_bwd_ln_packed_bf16 if first is not None else lib.vrwkv_mix_bwd_ln_carry_bf16
        rc = entry(*head, *carry, dy.data_ptr(), dmu.data_ptr(), ws.data_ptr(), st)
        assert rc == 0, rc
        ws2 = torch.empty(lib.vrwkv_add_ln_ws_floats(n, C), device="cuda")
        rc = lib.vrwkv_add_ln_bwd_bf16(n, C, dy.data_ptr(), _p(dres), xn.data_ptr(), mean.data_ptr(), rstd.data_ptr(), w.data_ptr(),
                                       dx.data_ptr(), dwb.data_ptr(), ws2.data_ptr(), st)
        assert rc == 0, rc
    torch.cuda.synchronize()
    return dx, dmu, dwb, dy_prev


rel = lambda a, r: float((a.double() - r.double()).norm() / r.double().norm())


def _autograd(xn, w, b, mus, douts, dres, second, y0, dyT, B, T, C):
    """fp64 autograd on the device from the rounded xn: LayerNorm -> shift from y0 -> lerps, plus <y[:, -1], dyT>."""
    xv = xn.double().requires_grad_(True)
    wv, bv = w.double().requires_grad_(True), b.double().requires_grad_(True)
    mv = [m.double().requires_grad_(True) for m in mus]
    yp = y0.double().requires_grad_(True)
    y = torch.nn.functional.layer_norm(xv, (C,), wv, bv, EPS).view(B, T, C)
    diff = torch.cat([yp.unsqueeze(1), y[:, :-1]], dim=1) - y
    loss = (y[:, -1] * dyT.double()).sum()
    for j, m in enumerate(mv):
        do = douts[j].double() + (second.double() if (second is not None and j == 3) else 0)
        loss = loss + ((y + diff * m) * do.view(B, T, C)).sum()
    loss.backward()
    return xv.grad + dres.double(), torch.stack([m.grad for m in mv]), torch.stack([wv.grad, bv.grad]), yp.grad


@pytest.mark.parametrize("M", [1, 6])
@pytest.mark.parametrize("B,T,C,cuts", CASES)
def test_carry_shift_entries(hip_lib, B, T, C, cuts, M):
    x, d, w, b, mus, douts, y0, dyT = _inputs(B, T, C, M, seed=B + T + C + M)
    dres, second = douts[M], (douts[M] if M == 6 else None)
    pieces = list(zip([0, *cuts], [*cuts, T]))
    # forward: the uncut launch (from zeros), the pieces chained
    whole = _fwd(hip_lib, B, T, C, M, x, d, w, b, mus, plain=True)
    null = _fwd(hip_lib, B, T, C, M, x, d, w, b, mus)
    assert torch.equal(null[0], whole[0]) and torch.equal(null[2], whole[2]) and torch.equal(null[3], whole[3])
    assert all(torch.equal(a_, b_) for a_, b_ in zip(null[1], whole[1]))
    y_prev, lasts = None, []
    for lo, hi in pieces:
        xn1, outs1, mean1, rstd1, y_last = _fwd(hip_lib, B, hi - lo, C, M, _cut(x, B, T, lo, hi), _cut(d, B, T, lo, hi), w, b, mus, y_prev, True)
        assert torch.equal(xn1, _cut(whole[0], B, T, lo, hi)), (lo, hi)
        assert torch.equal(mean1, _cut(whole[2], B, T, lo, hi)) and torch.equal(rstd1, _cut(whole[3], B, T, lo, hi)), (lo, hi)
        assert all(torch.equal(o1, _cut(o, B, T, lo, hi)) for o1, o in zip(outs1, whole[1])), (lo, hi)
        lasts.append(y_last)
        y_prev = y_last
    # backward: the uncut launch with carries at both ends, the pieces last to first
    xn, mean, rstd = whole[0], whole[2], whole[3]
    dx_w, dmu_w, dwb_w, dyp_w = _bwd(hip_lib, B, T, C, M, xn, mean, rstd, w, b, mus, douts, dres, second, y0, dyT, True)
    dx, dmu, dwb = torch.empty_like(xn), torch.zeros(M, C, device="cuda"), torch.zeros(2, C, device="cuda")
    dy_last = dyT
    for i in reversed(range(len(pieces))):
        lo, hi = pieces[i]
        cut = lambda t: _cut(t, B, T, lo, hi)
        dx1, dmu1, dwb1, dy_last = _bwd(hip_lib, B, hi - lo, C, M, cut(xn), cut(mean), cut(rstd), w, b, mus, [cut(t) for t in douts], cut(dres),
                                        cut(second) if second is not None else None, y0 if i == 0 else lasts[i - 1], dy_last, True)
        dx.view(B, T, C)[:, lo:hi] = dx1.view(B, hi - lo, C)
        dmu += dmu1
        dwb += dwb1
    assert torch.equal(dx, dx_w)
    assert torch.equal(dy_last, dyp_w)
    dx_r, dmu_r, dwb_r, dyp_r = _autograd(xn, w, b, mus, douts, dres, second, y0, dyT, B, T, C)
    for name, got, ref in (("dx", dx, dx_r), ("dmu", dmu, dmu_r), ("dwb", dwb, dwb_r), ("dmu uncut", dmu_w, dmu_r), ("dwb uncut", dwb_w, dwb_r),
                           ("dy_prev", dy_last, dyp_r)):
        e = rel(got, ref)
        print(f"[carry] M={M} ({B},{T},{C}) cuts {cuts}: {name} rel-RMS {e:.2e}")
        assert e < 6e-3, (name, e)
    # every carry pointer NULL: the existing entries, bit for bit
    plain_b = _bwd(hip_lib, B, T, C, M, xn, mean, rstd, w, b, mus, douts, dres, second, plain=True)
    null_b = _bwd(hip_lib, B, T, C, M, xn, mean, rstd, w, b, mus, douts, dres, second)
    assert all(torch.equal(a_, b_) for a_, b_ in zip(null_b[:3], plain_b[:3]))


FN_B, FN_T, FN_C = 2, 8, 64          # one wave, the smallest legal width: what the Python side can get wrong does not depend on size
FN_VARIANTS = ["plain", "first", "carry_none", "carry_bf16", "carry_fp32", "carry_nograd"]


@pytest.mark.parametrize("variant", FN_VARIANTS)
@pytest.mark.parametrize("has_delta", [True, False])
@pytest.mark.parametrize("M", [1, 6])
def test_add_ln_mix_is_the_entries(hip_lib, M, has_delta, variant):
    """fused.add_ln_mix (the autograd Function over the plain / _packed / _carry entries) against the drivers above on the same inputs: both sides
    run the same deterministic kernels, so every output and every gradient is torch.equal -- what can differ is the Python side's argument
    order, output count, needs_input_grad indices and dtypes.  Parameter gradients and y_prev.grad: the entries' fp32 results cast once."""
    from visualrwkv_amd import fused
    B, T, C = FN_B, FN_T, FN_C
    dup3 = M == 6
    x, d, w, b, mus, douts, y0, dyT = _inputs(B, T, C, M + 1, seed=100 + 10 * M + has_delta)     # M + 2 gradients: the lerps', the alias', xn's
    mus, (*g_out, g_dup, g_xn) = mus[:M], douts
    d = d if has_delta else None
    first = None
    if variant == "first":
        first = torch.zeros(B, T, dtype=torch.uint8)
        first[:, 0], first[0, 3] = 1, 1                      # a sample boundary at t = 3 of row 0
        first = first.view(-1).cuda()
    has_carry = variant.startswith("carry")
    y_prev = None
    if variant in ("carry_bf16", "carry_fp32", "carry_nograd"):
        y_prev = (y0.float() if variant == "carry_fp32" else y0.clone()).requires_grad_(variant != "carry_nograd")
    y0b = y0 if y_prev is not None else None

    ln = torch.nn.LayerNorm(C, eps=EPS).bfloat16().cuda()
    with torch.no_grad():
        ln.weight.copy_(w), ln.bias.copy_(b)
    xa = x.view(B, T, C).clone().requires_grad_(True)
    da = d.view(B, T, C).clone().requires_grad_(True) if has_delta else None
    ma = [m.view(1, 1, C).clone().requires_grad_(True) for m in mus]
    res = fused.add_ln_mix(xa, da, ln, ma, dup3, first, (y_prev,) if has_carry else None)
    assert len(res) == (3 if has_carry else 2)
    xn_a, outs_a = res[0], res[1]
    assert len(outs_a) == M + dup3

    xn, outs, mean, rstd, y_last = _fwd(hip_lib, B, T, C, M, x, d, w, b, mus, y0b, has_carry, first=first)
    assert torch.equal(xn_a.reshape(B * T, C), xn)
    assert all(torch.equal(a_.reshape(B * T, C), o_) for a_, o_ in zip(outs_a[:M], outs))
    if dup3:
        assert torch.equal(outs_a[M], outs_a[3]) and outs_a[M].data_ptr() == outs_a[3].data_ptr()
    if has_carry:
        assert res[2].dtype == torch.float32 and torch.equal(res[2], y_last.float())

    grads = [g_xn.view(B, T, C)] + [g.view(B, T, C) for g in g_out] + ([g_dup.view(B, T, C)] if dup3 else []) + ([dyT] if has_carry else [])
    torch.autograd.backward([xn_a, *outs_a, *res[2:]], grads)
    want_prev = y_prev is not None and y_prev.requires_grad
    dx, dmu, dwb, dy_prev = _bwd(hip_lib, B, T, C, M, xn, mean, rstd, w, b, mus, g_out, g_xn, g_dup if dup3 else None, y0b,
                                 dyT if has_carry else None, want_prev, first=first)
    assert torch.equal(xa.grad.reshape(B * T, C), dx)
    if has_delta:
        assert torch.equal(da.grad.reshape(B * T, C), dx)
    for j, m in enumerate(ma):
        assert m.grad.shape == m.shape and m.grad.dtype == torch.bfloat16 and torch.equal(m.grad.view(C), dmu[j].bfloat16()), j
    assert torch.equal(ln.weight.grad, dwb[0].bfloat16()) and torch.equal(ln.bias.grad, dwb[1].bfloat16())
    if want_prev:
        assert y_prev.grad.dtype == y_prev.dtype and torch.equal(y_prev.grad, dy_prev.to(y_prev.dtype))
    elif y_prev is not None:
        assert y_prev.grad is None


def test_add_ln_mix_refuses_first_with_a_carry(hip_lib):
    from visualrwkv_amd import fused
    B, T, C = FN_B, FN_T, FN_C
    x, d, w, b, mus, _, y0, _ = _inputs(B, T, C, 1, seed=7)
    ln = torch.nn.LayerNorm(C, eps=EPS).bfloat16().cuda()
    first = torch.zeros(B * T, dtype=torch.uint8, device="cuda")
    with pytest.raises(NotImplementedError):
        fused.add_ln_mix(x.view(B, T, C), d.view(B, T, C), ln, mus, False, first, (y0,))
