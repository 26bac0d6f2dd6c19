"""vrwkv_wkv6_forward_state_bf16 / vrwkv_wkv6_backward_state_bf16 (csrc/wkv6_capi.hip; the STATE instantiations of fwd6_kernel,
bwd6_kernel and bwd6_kernel_v2) called through ctypes: the SAME test bodies on the host lockstep emulator (tests/emu/emu_wkv6_capi.cpp
compiles the launchers whole) and on the MI355X (`gpu` marker), against fp64 autograd through oracle.wkv6_oracle.wkv6_naive(state0=)
with loss sum(y gy) + sum(S_T d_state_T).

States are (B,H,64,64) fp32 [key j][value i]; the oracle's S[i][j] is the transpose.

Bounds.  y 3e-3, gr gk gv gw 4e-3, gu 8e-3 (emulator) / 1e-2 (GPU) and state_T 2e-5 are the ones tests/test_emulated_wkv6.py and
tests/test_wkv6_gpu.py::test_op_matches_oracle hold the plain kernels to.  d_state0 is a new fp32 output: its rel-RMS against fp64 was
measured on the emulator over SHAPES and both backward kernels, worst 2.024e-6 (D_STATE0_MEASURED), and the bound is 4 x that, 8.1e-6 -- the
factor the project's emulator and GPU bounds of one quantity already stand in (test_ln_routed.py), for the hardware exponential and
FMA contraction that the emulator models with libm.
"""
import contextlib
import ctypes
import functools

import pytest
import torch

from oracle.wkv6_oracle import make_inputs6, wkv6_naive
from oracle.wkv7_oracle import rel_rms

SHAPES = [(1, 1, 1), (2, 16, 2), (2, 17, 2), (2, 37, 3), (1, 80, 2)]      # ragged chunk | full chunk | + 1 token | 3 chunks, ragged | 5 chunks
Y_TOL, G_TOL, ST_TOL = 3e-3, 4e-3, 2e-5
GU_TOL = {"emu": 8e-3, "gpu": 1e-2}
D_STATE0_MEASURED = 2.03e-6       # emulator, worst of SHAPES x {four-wave, three-role}: 2.024e-6 at (2,16,2); (1,1,1) 3.4e-8, the others 1.9-2.0e-6
D_STATE0_TOL = 4 * D_STATE0_MEASURED
EINVAL, ESHAPE, EALIGN = -1, -2, -3


def P(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


class Backend:
    def __init__(self, kind, lib):
        self.kind, self.lib = kind, lib
        self.dev = "cuda" if kind == "gpu" else "cpu"

    def to(self, *ts):
        return [t.to(self.dev).contiguous() if t is not None else None for t in ts]

    def sync(self):
        if self.kind == "gpu":
            torch.cuda.synchronize()

    def zeros(self, *shape, dtype=torch.float32):
        return torch.zeros(*shape, dtype=dtype, device=self.dev)

    def forward(self, r, k, v, ew, u, state0=None, want_state=True, entry="state"):
        """r k v ew (B,T,H,64), u (H,64) on the backend's device -> y, state_T, ckpt (CPU copies)"""
        B, T, H, _ = r.shape
        y = torch.zeros_like(r)
        ck = self.zeros(B * H, (T + 15) // 16, 64, 64)
        fin = self.zeros(B, H, 64, 64) if want_state else None
        if entry == "state":
            rc = self.lib.vrwkv_wkv6_forward_state_bf16(B, T, H * 64, H, P(r), P(k), P(v), P(ew), P(u), P(state0), P(y), P(fin), P(ck), None)
        else:
            rc = self.lib.vrwkv_wkv6_forward_bf16(B, T, H * 64, H, P(r), P(k), P(v), P(ew), P(u), P(y), P(ck), None)
        assert rc == 0, rc
        self.sync()
        return y, fin, ck

    def backward(self, r, k, v, ew, u, gy, ck, d_state_T=None, want_d0=True, entry="state"):
        B, T, H, _ = r.shape
        outs = [torch.zeros_like(r) for _ in range(4)]
        gu = self.zeros(B, H * 64, dtype=torch.bfloat16)
        d0 = self.zeros(B, H, 64, 64) if want_d0 else None
        if entry == "state":
            rc = self.lib.vrwkv_wkv6_backward_state_bf16(B, T, H * 64, H, P(r), P(k), P(v), P(ew), P(u), P(gy), P(ck), P(d_state_T),
                                                         *[P(o) for o in outs], P(gu), P(d0), None)
        else:
            rc = self.lib.vrwkv_wkv6_backward_bf16(B, T, H * 64, H, P(r), P(k), P(v), P(ew), P(u), P(gy), P(ck), *[P(o) for o in outs], P(gu), None)
        assert rc == 0, rc
        self.sync()
        return outs, gu, d0

    @contextlib.contextmanager
    def variant(self, v):
        """1: four waves (wkv6_chunked.h), 2: three-role pipeline (wkv6_bwd_v2.h); reset to the default afterwards"""
        assert self.lib.vrwkv_wkv6_set_backward_variant(v) == 0
        try:
            yield
        finally:
            assert self.lib.vrwkv_wkv6_set_backward_variant(-1) == 0


@pytest.fixture(scope="module", params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def be(request):
    if request.param == "emu":
        return Backend("emu", request.getfixturevalue("emu_lib"))
    from visualrwkv_amd import hip_lib
    return Backend("gpu", hip_lib.load())


@functools.lru_cache(maxsize=None)
def case(B, T, H, seed=0):
    """Inputs (the reference's own distributions; state0, d_state_T ~ U(-1, 1)) and the fp64 reference, computed once per shape."""
    r, k, v, w, u, gy = make_inputs6(B, T, H, seed=seed or 7000 + 10 * T + H)
    g = torch.Generator().manual_seed(T + 31 * H)
    s0 = torch.rand(B, H, 64, 64, generator=g) * 2 - 1
    dsT = torch.rand(B, H, 64, 64, generator=g) * 2 - 1
    ew = (-torch.exp(w.float())).contiguous()
    leaves = [x.double().requires_grad_(True) for x in (r, k, v, w, u)]
    st = s0.double().transpose(-1, -2).contiguous().requires_grad_(True)          # the oracle's [i][j]
    y, S = wkv6_naive(*leaves, state0=st)
    ((y * gy.double()).sum() + (S * dsT.double().transpose(-1, -2)).sum()).backward()
    ref = dict(y=y.detach(), state_T=S.detach().transpose(-1, -2), gr=leaves[0].grad, gk=leaves[1].grad, gv=leaves[2].grad, gw=leaves[3].grad,
               gu=leaves[4].grad, d_state0=st.grad.transpose(-1, -2))
    return dict(r=r, k=k, v=v, ew=ew, u=u, gy=gy, s0=s0, dsT=dsT), ref


def check(be, tag, ref, y=None, state_T=None, grads=None, gu=None, d0=None):
    figs = {}
    if y is not None:
        figs["y"] = (rel_rms(y.cpu().double(), ref["y"]), Y_TOL)
    if state_T is not None:
        figs["state_T"] = (rel_rms(state_T.cpu().double(), ref["state_T"]), ST_TOL)
    if grads is not None:
        for n, o in zip(("gr", "gk", "gv", "gw"), grads):
            figs[n] = (rel_rms(o.cpu().double(), ref[n]), G_TOL)
    if gu is not None:
        H = ref["gu"].shape[0]
        figs["gu"] = (rel_rms(gu.cpu().double().sum(0).view(H, 64), ref["gu"]), GU_TOL[be.kind])     # per-sample bf16 rows, summed as the reference does
    if d0 is not None:
        figs["d_state0"] = (rel_rms(d0.cpu().double(), ref["d_state0"]), D_STATE0_TOL)
    print(f"[wkv6 state] {be.kind} {tag}: " + "  ".join(f"{n} {e:.3e}" for n, (e, _) in figs.items()))
    for n, (e, tol) in figs.items():
        assert e < tol, (tag, n, e, tol)


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("B,T,H", SHAPES)
def test_state_entries_against_fp64(be, B, T, H, variant):
    """d_state0 rel-RMS against fp64 on the emulator, both backward kernels alike: (1,1,1) 3.44e-8, (2,16,2) 2.024e-6, (2,17,2) 1.973e-6,
    (2,37,3) 2.021e-6, (1,80,2) 1.948e-6 -> worst 2.024e-6, bound 4 x = 8.1e-6 (D_STATE0_TOL)."""
    ins, ref = case(B, T, H)
    r, k, v, ew, u, gy, s0, dsT = be.to(*[ins[n] for n in ("r", "k", "v", "ew", "u", "gy", "s0", "dsT")])
    y, fin, ck = be.forward(r, k, v, ew, u, s0)
    assert torch.equal(ck.view(B, H, -1, 64, 64)[:, :, 0], s0)                 # the checkpoint of chunk 0 is state0: the backward needs no other copy
    with be.variant(variant):
        grads, gu, d0 = be.backward(r, k, v, ew, u, gy, ck, dsT)
    check(be, f"{B}x{T}x{H} variant {variant}", ref, y, fin, grads, gu, d0)


@pytest.mark.parametrize("variant", [1, 2])
def test_null_state_pointers_are_the_plain_entries(be, variant):
    B, T, H = 2, 37, 3
    ins, _ = case(B, T, H)
    r, k, v, ew, u, gy = be.to(*[ins[n] for n in ("r", "k", "v", "ew", "u", "gy")])
    y0, _, ck0 = be.forward(r, k, v, ew, u, entry="plain")
    y1, _, ck1 = be.forward(r, k, v, ew, u, None, want_state=False)
    assert torch.equal(y0, y1) and torch.equal(ck0, ck1)
    with be.variant(variant):
        g0, gu0, _ = be.backward(r, k, v, ew, u, gy, ck0, entry="plain")
        g1, gu1, _ = be.backward(r, k, v, ew, u, gy, ck0, None, want_d0=False)
    for n, a, b in zip(("gr", "gk", "gv", "gw"), g0, g1):
        assert torch.equal(a, b), n
    assert torch.equal(gu0, gu1)


def test_zero_state0_is_the_plain_forward(be):
    B, T, H = 2, 37, 3
    ins, _ = case(B, T, H)
    r, k, v, ew, u = be.to(*[ins[n] for n in ("r", "k", "v", "ew", "u")])
    y0, _, ck0 = be.forward(r, k, v, ew, u, entry="plain")
    y1, _, ck1 = be.forward(r, k, v, ew, u, be.zeros(B, H, 64, 64))
    assert torch.equal(y0, y1) and torch.equal(ck0, ck1)


@pytest.mark.parametrize("cut", [16, 32])
def test_forward_split_identity(be, cut):
    """T = 48 as 16 + 32 and 32 + 16 with the state handed over: a chunk's decay scan reads only its own ew and S crosses the cut as the same
    fp32 values, so y and state_T equal the unsplit run's bit for bit."""
    B, T, H = 2, 48, 2
    ins, _ = case(B, T, H)
    r, k, v, ew, u, s0 = be.to(*[ins[n] for n in ("r", "k", "v", "ew", "u", "s0")])
    y, fin, _ = be.forward(r, k, v, ew, u, s0)
    a = [x[:, :cut].contiguous() for x in (r, k, v, ew)]
    b = [x[:, cut:].contiguous() for x in (r, k, v, ew)]
    ya, mid, _ = be.forward(*a, u, s0)
    yb, fin2, _ = be.forward(*b, u, mid)
    assert torch.equal(torch.cat([ya, yb], dim=1), y)
    assert torch.equal(fin2, fin)


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("cut", [16, 32])
def test_backward_chain_against_fp64(be, cut, variant):
    """d_state0 of the later part is d_state_T of the earlier one."""
    B, T, H = 2, 48, 2
    ins, ref = case(B, T, H)
    r, k, v, ew, u, gy, s0, dsT = be.to(*[ins[n] for n in ("r", "k", "v", "ew", "u", "gy", "s0", "dsT")])
    a = [x[:, :cut].contiguous() for x in (r, k, v, ew)]
    b = [x[:, cut:].contiguous() for x in (r, k, v, ew)]
    ya, mid, cka = be.forward(*a, u, s0)
    yb, fin, ckb = be.forward(*b, u, mid)
    with be.variant(variant):
        gb, gub, dmid = be.backward(*b, u, gy[:, cut:].contiguous(), ckb, dsT)
        ga, gua, d0 = be.backward(*a, u, gy[:, :cut].contiguous(), cka, dmid)
    grads = [torch.cat([x, y_], dim=1) for x, y_ in zip(ga, gb)]
    gu = (gua.float() + gub.float())                                                # per-sample rows of the two parts, summed in fp32
    check(be, f"chain {cut}+{T - cut} variant {variant}", ref, torch.cat([ya, yb], dim=1), fin, grads, gu, d0)


def test_bad_state_arguments_are_refused(be):
    """The plain entries' checks and codes: nothing is launched."""
    B, T, H = 1, 16, 1
    x = be.zeros(B, T, H, 64, dtype=torch.bfloat16)
    ew, u = be.zeros(B, T, H, 64), be.zeros(H, 64, dtype=torch.bfloat16)
    st, ck = be.zeros(B, H, 64 * 64 + 4), be.zeros(B * H, 1, 64, 64)
    ok = P(st)
    mis = ctypes.c_void_p(st.data_ptr() + 4)
    lib = be.lib
    fwd = lambda C, Hh, s0, sT: lib.vrwkv_wkv6_forward_state_bf16(B, T, C, Hh, P(x), P(x), P(x), P(ew), P(u), s0, P(x), sT, P(ck), None)
    bwd = lambda C, Hh, dT, d0: lib.vrwkv_wkv6_backward_state_bf16(B, T, C, Hh, P(x), P(x), P(x), P(ew), P(u), P(x), P(ck), dT,
                                                                  P(x), P(x), P(x), P(x), P(u), d0, None)
    assert fwd(64, 1, mis, ok) == EALIGN and fwd(64, 1, ok, mis) == EALIGN
    assert bwd(64, 1, mis, ok) == EALIGN and bwd(64, 1, ok, mis) == EALIGN
    assert fwd(128, 1, ok, ok) == ESHAPE and bwd(128, 1, ok, ok) == ESHAPE      # a state sized for another head count: C != 64 H
    assert fwd(64, 0, ok, ok) == EINVAL and bwd(64, 0, ok, ok) == EINVAL
