"""What the stream entries outside the glue, LayerNorm, decode and weight-gradient families refuse, by return code, through the C ABI on the
two backends of tests/test_glue_shapes.py with the same bodies: the host lockstep emulator (CPU tensors; tests/emu compiles fused_ops.hip,
visual_ops.hip, wkv6_capi.hip and image_ops.hip whole) and the product library on an MI355X (`gpu` marker).

  vrwkv_transpose_bf16 (fused_ops.hip), vrwkv_adaptive_pool_bf16 / vrwkv_gate_fwd_bf16 / vrwkv_gate_bwd_bf16 / vrwkv_gelu_bf16 (visual_ops.hip),
  vrwkv_wkv6_forward(_state)_bf16 / vrwkv_wkv6_backward(_state)_bf16 (wkv6_capi.hip, both backward variants), vrwkv_resize_normalize_u8 (image_ops.hip)

Every table starts from the smallest valid call of its entry; a case is one change to it (a count, a width, a NULL pointer, a pointer moved by
8 bytes), then the pairs that show which check comes first.  Asserted per case: the return code, and that everything the entry would write is
NaN before the call and after it -- a refused call launches nothing.  The valid call then returns 0.  The codes are read off the entries as
they stand (counts and NULL -> VRWKV_EINVAL, shapes -> VRWKV_ESHAPE, 16-byte alignment -> VRWKV_EALIGN where the entry tests it; the visual_ops
entries test none), not derived from what they ought to be.  No case depends on being refused to stay in bounds: every buffer is 32 KiB, the
largest tensor of a valid call 16 KiB.
"""
import ctypes

import pytest
import torch

from tests.test_glue_shapes import BACKENDS, F32, I, L, VP, Backend, bits

EINVAL, ESHAPE, EALIGN = -1, -2, -3                      # include/visualrwkv_hip.h
BUF = 8192                                               # floats per buffer
NAN = float("nan")


@pytest.fixture
def be(request, backend):
    return Backend(request, backend)


class Table:
    """One entry: `sig` names its arguments in order (a scalar as name:I / name:L, anything else a pointer; > marks what the entry writes, ? a
    pointer the valid call leaves NULL).  Pointers read are zeros, pointers written one NaN row of `outs` each."""

    def __init__(self, be, fn, sig, **scalars):
        self.be, self.fn = be, fn
        self.zeros = torch.zeros(BUF, dtype=torch.float32, device=be.dev)
        self.names, self.types, self.base = [], [], {}
        args = sig.split()
        self.outs = torch.full((sum(a.startswith(">") for a in args), BUF), NAN, dtype=torch.float32, device=be.dev)
        k = 0
        for a in args:
            n, _, t = a.strip(">?").partition(":")
            self.names.append(n)
            self.types.append({"I": I, "L": L, "": VP}[t])
            if t:
                self.base[n] = scalars[n]
            elif a.endswith("?"):
                self.base[n] = None
            elif a.startswith(">"):
                self.base[n] = self.outs[k].data_ptr()
                k += 1
            else:
                self.base[n] = scalars.get(n, self.zeros.data_ptr())
        self.pointers = [n for n, t in zip(self.names, self.types) if t is VP]

    def rc(self, **change):
        a = {**self.base, **change}
        vals = [a[n] if t is not VP or a[n] is None or not isinstance(a[n], int) else VP(a[n]) for n, t in zip(self.names, self.types)]
        return self.be.rc(self.fn, self.types, *vals)

    def off(self, n, by=8):
        return {n: self.base[n] + by}

    def refused(self, want, **change):
        rc = self.rc(**change)
        assert rc == want, (self.fn, change, rc)
        assert bool(torch.isnan(self.outs).all()), (self.fn, change, "a refused call wrote")

    def accepted(self, **change):
        assert self.rc(**change) == 0, (self.fn, change)
        self.outs.fill_(NAN)


@pytest.mark.parametrize("backend", BACKENDS)
def test_rejects_transpose(backend, be):
    t = Table(be, "vrwkv_transpose_bf16", "rows:L cols:L in >out", rows=64, cols=64)
    for k in ("rows", "cols"):
        t.refused(EINVAL, **{k: 0})
        t.refused(ESHAPE, **{k: 32})
        t.refused(ESHAPE, **{k: 96})
    for p in ("in", "out"):
        t.refused(EINVAL, **{p: None})
        t.refused(EALIGN, **t.off(p))
        t.refused(ESHAPE, rows=32, **t.off(p))                       # the shape before the alignment
        t.refused(EINVAL, rows=32, **{p: None})                      # NULL before the shape
    t.refused(EINVAL, **{"in": None}, **t.off("out"))                # NULL before the alignment
    t.accepted()


@pytest.mark.parametrize("backend", BACKENDS)
def test_rejects_adaptive_pool(backend, be):
    t = Table(be, "vrwkv_adaptive_pool_bf16", "B:I side_in:I side_out:I D:I x >y", B=1, side_in=2, side_out=1, D=8)
    for k in ("B", "side_in", "side_out"):
        t.refused(EINVAL, **{k: 0})
        t.refused(EINVAL, D=12, **{k: 0})                            # a count before the width
    t.refused(ESHAPE, D=0)
    t.refused(ESHAPE, D=12)
    for p in ("x", "y"):
        t.refused(EINVAL, **{p: None})
        t.refused(EINVAL, D=12, **{p: None})
    t.accepted()
    t.accepted(**t.off("x"), **t.off("y"))                           # no alignment test in this entry: 8 bytes off is taken


@pytest.mark.parametrize("backend", BACKENDS)
def test_rejects_gate(backend, be):
    fwd = Table(be, "vrwkv_gate_fwd_bf16", "n:L x g >out", n=8)
    bwd = Table(be, "vrwkv_gate_bwd_bf16", "n:L x g dout >dg >dx?", n=8)
    for t, required in ((fwd, ("x", "g", "out")), (bwd, ("x", "g", "dout", "dg"))):
        t.refused(EINVAL, n=0)
        t.refused(ESHAPE, n=12)
        for p in required:
            t.refused(EINVAL, **{p: None})
            t.refused(EINVAL, n=12, **{p: None})                     # NULL before the shape
        t.accepted()
    # dx is optional: without it, dg is what the two-output call writes
    g = be.gen(11)
    x, gg, dout = (torch.randn(8, generator=g, device=be.dev).bfloat16() for _ in range(3))
    dg1, dg2, dx = (torch.full((16,), NAN, dtype=torch.bfloat16, device=be.dev) for _ in range(3))
    ptr = dict(x=x.data_ptr(), g=gg.data_ptr(), dout=dout.data_ptr())
    assert bwd.rc(**ptr, dg=dg1.data_ptr()) == 0 and bwd.rc(**ptr, dg=dg2.data_ptr(), dx=dx.data_ptr()) == 0
    assert bool(torch.isfinite(dg1[:8].float()).all()) and bool(torch.isfinite(dx[:8].float()).all())
    assert torch.equal(bits(dg1), bits(dg2)), "dg depends on dx being asked for"
    assert bool(torch.isnan(dg1[8:].float()).all()) and bool(torch.isnan(dx[8:].float()).all()), "written past n"


@pytest.mark.parametrize("backend", BACKENDS)
def test_rejects_gelu(backend, be):
    t = Table(be, "vrwkv_gelu_bf16", "n:L x >y tanh:I", n=8, tanh=0)
    for tanh in (0, 1):
        t.refused(EINVAL, n=0, tanh=tanh)
        t.refused(ESHAPE, n=12, tanh=tanh)
        t.refused(EINVAL, x=None, tanh=tanh)
        t.refused(EINVAL, y=None, tanh=tanh)
        t.refused(EINVAL, n=12, x=None, tanh=tanh)
        t.refused(ESHAPE, n=8 * 256 * 2 ** 31, tanh=tanh)           # more workgroups than a grid dimension holds
        t.accepted(tanh=tanh)
    # in place, as the towers call it (moved here from test_emulated_misc.py, which ran it on the emulator alone)
    y = t.base["y"]
    assert t.rc(n=12, x=y) == -2 and t.rc(n=0, x=y) == -1 and t.rc(n=8, x=None) == -1
    assert bool(torch.isnan(t.outs).all())


WKV6_IN = "B:I T:I C:I H:I r k v ew u"
WKV6 = {
    "vrwkv_wkv6_forward_bf16": (WKV6_IN + " >y >s_ckpt", ()),
    "vrwkv_wkv6_forward_state_bf16": (WKV6_IN + " state0 >y >state_T >s_ckpt", ("state0", "state_T")),
    "vrwkv_wkv6_backward_bf16": (WKV6_IN + " gy s_ckpt >gr >gk >gv >gw >gu", ()),
    "vrwkv_wkv6_backward_state_bf16": (WKV6_IN + " gy s_ckpt d_state_T >gr >gk >gv >gw >gu >d_state0", ("d_state_T", "d_state0")),
}


WKV6_CASES = [(e, v) for e in WKV6 for v in ((1, 2) if "backward" in e else (None,))]          # 1: four waves, 2: three-role pipeline (the default)


@pytest.mark.parametrize("entry,variant", WKV6_CASES, ids=[e[11:-5] + (f"-v{v}" if v else "") for e, v in WKV6_CASES])
@pytest.mark.parametrize("backend", BACKENDS)
def test_rejects_wkv6(backend, be, entry, variant):
    """B 1, T 16, H 1, C 64.  The forward's s_ckpt and the state pointers may be NULL; given, they are held to 16 bytes like the rest."""
    sig, optional = WKV6[entry]
    t = Table(be, entry, sig, B=1, T=16, C=64, H=1)
    optional += ("s_ckpt",) if "forward" in entry else ()
    if variant is not None:
        assert be.lib.vrwkv_wkv6_set_backward_variant(variant) == 0
    try:
        for k in ("B", "T", "H"):
            t.refused(EINVAL, **{k: 0})
        t.refused(EINVAL, B=0, C=32)                                 # a count before the shape
        for c in (32, 128, 0):
            t.refused(ESHAPE, C=c)
        t.refused(ESHAPE, H=2)
        for p in t.pointers:
            t.refused(EALIGN, **t.off(p))
            t.refused(ESHAPE, C=32, **t.off(p))
            if p in optional:
                continue
            t.refused(EINVAL, **{p: None})
            t.refused(ESHAPE, C=32, **{p: None})                     # the shape before NULL
            other = next(q for q in t.pointers if q != p)
            t.refused(EINVAL, **{p: None}, **t.off(other))           # NULL before the alignment
        t.accepted()
        if optional:
            t.accepted(**{p: None for p in optional})
    finally:
        if variant is not None:
            assert be.lib.vrwkv_wkv6_set_backward_variant(-1) == 0


@pytest.mark.parametrize("backend", BACKENDS)
def test_rejects_resize_normalize(backend, be):
    """4 x 4 -> S 2.  mean3 and std3 are host arrays: the entry reads them before it launches."""
    mean, std = (F32 * 3)(0.5, 0.4, 0.3), (F32 * 3)(0.2, 0.25, 0.3)
    for f32 in (0, 1):
        t = Table(be, "vrwkv_resize_normalize_u8", "H:I W:I src S:I mean3 std3 >dst f32:I", H=4, W=4, S=2, f32=f32, mean3=mean, std3=std)
        for k in ("H", "W", "S"):
            t.refused(EINVAL, **{k: 0})
        for p in ("src", "mean3", "std3", "dst"):
            t.refused(EINVAL, **{p: None})
        for c in range(3):
            for bad in (0.0, -1.0, NAN):
                s = (F32 * 3)(0.2, 0.25, 0.3)
                s[c] = bad
                t.refused(EINVAL, std3=s)
        t.refused(ESHAPE, H=2 ** 20, W=4)                            # a down-sampling ratio whose taps do not fit the LDS
        t.refused(EINVAL, H=2 ** 20, std3=(F32 * 3)(0.2, 0.25, 0.0))  # std3 before the LDS size
        t.accepted()
