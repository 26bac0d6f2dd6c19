"""Packed rows on the host lockstep emulator: the PACKED instantiations of csrc/wkv7_fwd_v4.h and csrc/wkv7_bwd_v8.h (schedules 8 and 9),
the C entries vrwkv_wkv7_forward_packed_bf16 / vrwkv_wkv7_backward_packed_bf16 and the autograd node on top of them.

A packed row is several samples end to end, each a whole number of 16-token chunks.  Two statements are checked for every sample:
  * against fp64 autograd through the oracle recurrence run on the sample's slice alone, within the limits of the existing WKV7 parity
    tests (tests/state_ref.py);
  * against the SAME emulated kernels run on the sample's slice alone: bit-identical (torch.equal) y, sa, checkpoints and gradients.  A
    chunk step is a function of the incoming state, the chunk's rows and the incoming dL/dS only, and the kernels reset exactly those two
    at a flagged chunk.  ONE operation differs, on purpose, and only dw sees it: the tail of the packed backward writes dw = 0 at the first
    token of a flagged chunk (tail8's `zero_first`).  That is the exact value -- w of that token multiplies the zero state before it, and
    the fp64 reference has 0.0 there -- where the plain kernel, which cannot know that a launch starts from zero, leaves the cancellation
    residue of its sum (~5e-5 against |dw| ~ 0.3).  dw is therefore bit-identical on every other token, exactly 0 on those, and held to the
    fp64 limits as a whole; the other five gradients and the forward outputs are bit-identical throughout.
"""
import contextlib
import ctypes

import pytest
import torch

from oracle.wkv7_oracle import make_inputs
from tests.parity import bf16_close
from tests.state_ref import FLIP_W, FLIP_Y, NAMES, P, TOL, check_grads, reference

B, H, T = 2, 2, 160
LAYOUTS = [
    [[48, 16, 96], [160]],
    [[16] * 10, [80, 80]],
    [[144, 16], [16, 144]],
]


def _flags(layout, device="cpu"):
    from visualrwkv_amd.wkv7 import PackedLayout
    return PackedLayout(layout, T, device)


def _segments(layout):
    return [(b, t0, t1) for b, row in enumerate(layout) for t0, t1 in zip([sum(row[:i]) for i in range(len(row))], [sum(row[:i + 1]) for i in range(len(row))])]


def _fwd_packed(emu, ins, reset):
    Bn, Tn, Hn, _ = ins[0].shape
    y = torch.zeros_like(ins[3])
    s, sa = torch.zeros(Bn, Hn, Tn // 16, 64, 64), torch.zeros(Bn, Tn, Hn, 64)
    emu.emu_wkv7_forward_packed_v4(Bn, Tn, Hn, *[P(x) for x in ins], P(y), P(reset), P(s), P(sa))
    return y, s, sa


def _bwd_packed(emu, ins, dy, s, sa, reset, ahead):
    Bn, Tn, Hn, _ = ins[0].shape
    g = [torch.zeros_like(ins[0]) for _ in range(6)]
    emu.emu_wkv7_backward_packed_v8(Bn, Tn, Hn, *[P(x) for x in ins], P(dy), P(s), P(sa), P(reset), *[P(x) for x in g], ahead)
    return g


def _fwd_plain(emu, ins):
    Bn, Tn, Hn, _ = ins[0].shape
    y = torch.zeros_like(ins[3])
    s, sa = torch.zeros(Bn, Hn, Tn // 16, 64, 64), torch.zeros(Bn, Tn, Hn, 64)
    emu.emu_wkv7_forward(Bn, Tn, Hn, *[P(x) for x in ins], P(y), P(s), P(sa), 7)
    return y, s, sa


def _bwd_plain(emu, ins, dy, s, sa, ahead):
    Bn, Tn, Hn, _ = ins[0].shape
    g = [torch.zeros_like(ins[0]) for _ in range(6)]
    emu.emu_wkv7_backward_chunked(Bn, Tn, Hn, *[P(x) for x in ins], P(dy), P(s), P(sa), *[P(x) for x in g], 9 + ahead)
    return g


def _data(seed):
    *ins, dy = make_inputs(B, T, H, seed=seed)
    return tuple(ins), dy


def _reference_packed(ins, dy, layout):
    yr = torch.zeros(ins[0].shape, dtype=torch.float64)
    gr = [torch.zeros(ins[0].shape, dtype=torch.float64) for _ in range(6)]
    for b, t0, t1 in _segments(layout):
        y1, _, g1, _ = reference([x[b:b + 1, t0:t1].contiguous() for x in ins], dy[b:b + 1, t0:t1].contiguous())
        yr[b:b + 1, t0:t1] = y1
        for a_, b_ in zip(gr, g1):
            a_[b:b + 1, t0:t1] = b_
    return yr, gr


_RUNS = {}


def _run(emu, li, ahead):
    """One packed forward + backward and its fp64 reference per (layout, schedule), shared by the tests below."""
    if (li, ahead) not in _RUNS:
        ins, dy = _data(100 + 10 * li + ahead)
        lay = _flags(LAYOUTS[li])
        y, s, sa = _fwd_packed(emu, ins, lay.chunk_reset)
        g = _bwd_packed(emu, ins, dy, s, sa, lay.chunk_reset, ahead)
        _RUNS[(li, ahead)] = (ins, dy, lay, y, s, sa, g, _reference_packed(ins, dy, LAYOUTS[li]))
    return _RUNS[(li, ahead)]


def _figures(x, ref):
    xr, rr = x.float().reshape(-1), ref.double().reshape(-1).float().bfloat16().float()
    return float((xr - rr).double().norm() / rr.double().norm().clamp_min(1e-30)), float((xr != rr).float().mean())


@pytest.mark.parametrize("ahead", [0, 1])
@pytest.mark.parametrize("li", range(len(LAYOUTS)))
def test_packed_rows_against_fp64(emu_lib, li, ahead):
    """y and the six gradients of the packed rows against the fp64 reference run on every segment's slice alone, concatenated, within the
    limits of tests/state_ref.py.

    dw: 1 / (tokens of a sample) of its elements belong to a first token, where the reference is exactly 0; the packed backward writes that
    0 (module docstring).  With the plain kernel's residue in their place every one of them counts as a flip of bf16_close whatever its
    size: 5.2 % on layout 1 against FLIP_W = 3 %, 1.3-2.1 % on the other tokens."""
    ins, dy, lay, y, s, sa, g, (yr, gr) = _run(emu_lib, li, ahead)
    for n, a_, b_ in zip(("y",) + NAMES, [y] + g, [yr] + gr):
        print(f"[packed] layout {li} schedule {8 + ahead} {n}: rel-RMS %.3e flips %.4f" % _figures(a_, b_))
    bf16_close(y, yr, f"layout {li} y", tol=TOL, max_flip=FLIP_Y)
    check_grads(g, gr, f"layout {li} schedule {8 + ahead}")


@pytest.mark.parametrize("ahead", [0, 1])
@pytest.mark.parametrize("li", range(len(LAYOUTS)))
def test_dw_of_a_first_token_is_exactly_zero(emu_lib, li, ahead):
    """Where the fp64 reference is exactly 0 the packed backward writes 0; nothing else of dw is touched (the bit-identity test below)."""
    ins, dy, lay, y, s, sa, g, (yr, gr) = _run(emu_lib, li, ahead)
    first = lay.first.view(B, T).bool()
    assert float(gr[0][first].abs().max()) == 0.0
    assert float(g[0][first].float().abs().max()) == 0.0
    assert float(g[0][~first].float().abs().min()) > 0.0


@pytest.mark.parametrize("ahead", [0, 1])
@pytest.mark.parametrize("li", range(len(LAYOUTS)))
def test_packed_rows_bit_identical_to_launches_per_segment(emu_lib, li, ahead):
    """Resets next to both ends of a row, runs of one-chunk samples shorter than the pipeline depth, a row without a reset: y, sa, the
    checkpoints and the gradients of every segment are those of the same kernels launched on the segment alone -- dw on every token but the
    segment's first, where the packed tail writes the exact 0 in place of the plain kernel's residue (module docstring)."""
    ins, dy, lay, y, s, sa, g, _ = _run(emu_lib, li, ahead)
    for b, t0, t1 in _segments(LAYOUTS[li]):
        cut = [x[b:b + 1, t0:t1].contiguous() for x in ins]
        dyc = dy[b:b + 1, t0:t1].contiguous()
        what = f"layout {li} schedule {8 + ahead} row {b} tokens {t0}:{t1}"
        y1, s1, sa1 = _fwd_plain(emu_lib, cut)
        g1 = _bwd_plain(emu_lib, cut, dyc, s1, sa1, ahead)
        assert torch.equal(y[b:b + 1, t0:t1], y1), f"{what} y"
        assert torch.equal(sa[b:b + 1, t0:t1], sa1), f"{what} sa"
        assert torch.equal(s[b:b + 1, :, t0 // 16:t1 // 16], s1), f"{what} s_ckpt"
        for n, a_, b_ in zip(NAMES, g, g1):
            skip = 1 if n == "dw" else 0
            assert torch.equal(a_[b:b + 1, t0 + skip:t1], b_[:, skip:]), f"{what} {n}"
        assert float(g[0][b, t0].float().abs().max()) == 0.0 and float(g1[0][0, 0].float().abs().max()) > 0.0, f"{what} dw of the first token"


@pytest.mark.parametrize("ahead", [0, 1])
@pytest.mark.parametrize("null", [False, True])
def test_no_resets_is_the_plain_kernel(emu_lib, null, ahead):
    ins, dy = _data(7 + ahead)
    reset = None if null else torch.zeros(B, T // 16, dtype=torch.uint8)
    y, s, sa = _fwd_packed(emu_lib, ins, reset)
    y1, s1, sa1 = _fwd_plain(emu_lib, ins)
    assert torch.equal(y, y1) and torch.equal(s, s1) and torch.equal(sa, sa1)
    g = _bwd_packed(emu_lib, ins, dy, s, sa, reset, ahead)
    g1 = _bwd_plain(emu_lib, ins, dy, s1, sa1, ahead)
    for n, a_, b_ in zip(NAMES, g, g1):
        assert torch.equal(a_, b_), n


def test_forward_without_by_products(emu_lib):
    ins, _ = _data(3)
    lay = _flags(LAYOUTS[0])
    y, _, _ = _fwd_packed(emu_lib, ins, lay.chunk_reset)
    y2 = torch.zeros_like(y)
    emu_lib.emu_wkv7_forward_packed_v4(B, T, H, *[P(x) for x in ins], P(y2), P(lay.chunk_reset), None, None)
    assert torch.equal(y, y2)


def _shim(emu):
    V = lambda p: ctypes.c_void_p(p) if p else None

    class Shim:                                              # csrc/wkv7_capi.hip itself, compiled for the host
        @staticmethod
        def vrwkv_wkv7_forward_packed_bf16(Bn, Tn, Hn, *rest):
            fn = emu.vrwkv_wkv7_forward_packed_bf16
            fn.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 11
            return fn(Bn, Tn, Hn, *[V(p) for p in rest])

        @staticmethod
        def vrwkv_wkv7_backward_packed_bf16(Bn, Tn, Hn, *rest):
            fn = emu.vrwkv_wkv7_backward_packed_bf16
            fn.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 17
            return fn(Bn, Tn, Hn, *[V(p) for p in rest])

        @staticmethod
        def vrwkv_strerror(code):
            return b"emulated"
    return Shim


@pytest.fixture
def emulated_op(emu_lib, monkeypatch):
    from visualrwkv_amd import hip_lib, wkv7
    monkeypatch.setattr(hip_lib, "load", lambda: _shim(emu_lib))
    monkeypatch.setattr(wkv7, "_native", lambda t: True)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    monkeypatch.setattr(hip_lib, "launch_stream", lambda device: 0)
    return wkv7


@pytest.mark.parametrize("variant", [-1, 9, 5])           # -1: schedule 8 at this size; 5: no packed kernel -> the plain op per segment
@pytest.mark.parametrize("recompute", [False, True])
def test_autograd_node_through_the_c_entry(emu_lib, emulated_op, variant, recompute):
    layout = LAYOUTS[0]
    ins, dy = _data(40 + variant)
    yr, gr = _reference_packed(ins, dy, layout)
    lay = _flags(layout)
    views = [x.view(B, T, H * 64).clone().requires_grad_(True) for x in (ins[1], ins[0], *ins[2:])]       # (q, w, k, v, a, b) order
    assert emu_lib.vrwkv_wkv7_set_backward_variant(variant) == 0
    try:
        assert emu_lib.vrwkv_wkv7_resolve_variant(4, B, T, H) == 7
        assert emu_lib.vrwkv_wkv7_resolve_variant(5, B, T, H) == (8 if variant == -1 else variant)
        y = emulated_op.RUN_CUDA_RWKV7g_packed(*views, lay, recompute)
        (y.float() * dy.view(B, T, H * 64).float()).sum().backward()
        assert emu_lib.vrwkv_wkv7_last_variant(0) == 7
        if variant != 5:                                     # 5: VRWKV_ESHAPE, and the registered op (its CPU key here) runs per segment
            assert emu_lib.vrwkv_wkv7_last_variant(1) == (8 if variant == -1 else variant)
    finally:
        emu_lib.vrwkv_wkv7_set_backward_variant(-1)
    bf16_close(y.view(B, T, H, 64), yr, "y", tol=TOL, max_flip=FLIP_Y)
    got = [views[1].grad, views[0].grad, *[x.grad for x in views[2:]]]
    check_grads([x.view(B, T, H, 64) for x in got], gr, f"autograd node variant {variant} recompute {recompute}")


def test_no_gradient_wanted_skips_the_by_products(emulated_op):
    ins, _ = _data(9)
    lay = _flags(LAYOUTS[2])
    views = [x.view(B, T, H * 64) for x in (ins[1], ins[0], *ins[2:])]
    y = emulated_op.RUN_CUDA_RWKV7g_packed(*views, lay)
    assert not y.requires_grad
    leaves = [x.clone().requires_grad_(True) for x in views]
    y2 = emulated_op.RUN_CUDA_RWKV7g_packed(*leaves, lay)
    assert torch.equal(y, y2.detach())


def test_cpu_tensors_run_the_plain_op_per_segment():
    """No kernel of this file: the CPU key of torch.ops.wind_backstepping once per segment -- the statement the packed kernels are held to."""
    from visualrwkv_amd import wkv7
    layout = LAYOUTS[0]
    ins, dy = _data(21)
    yr, gr = _reference_packed(ins, dy, layout)
    views = [x.view(B, T, H * 64).clone().requires_grad_(True) for x in (ins[1], ins[0], *ins[2:])]
    y = wkv7.RUN_CUDA_RWKV7g_packed(*views, _flags(layout))
    (y.float() * dy.view(B, T, H * 64).float()).sum().backward()
    bf16_close(y.view(B, T, H, 64), yr, "y", tol=TOL, max_flip=FLIP_Y)
    got = [views[1].grad, views[0].grad, *[x.grad for x in views[2:]]]
    check_grads([x.view(B, T, H, 64) for x in got], gr, "CPU per segment")


def test_layout_validation():
    from visualrwkv_amd.wkv7 import PackedLayout
    lay = PackedLayout([[32, 16], [48]], 48)
    assert lay.chunk_reset.tolist() == [[1, 0, 1], [1, 0, 0]]
    assert lay.first.view(2, 48).nonzero().tolist() == [[0, 0], [0, 32], [1, 0]]
    assert lay.seg_id[0, 31] == 0 and lay.seg_id[0, 32] == 1 and lay.seg_id[1, 0] == 2 and lay.n_samples == 3
    assert lay.segments == [(0, 0, 32), (0, 32, 48), (1, 0, 48)]
    for bad in ([[32, 8, 8]], [[32]], [[48, 16]], [[]], [[0, 48]]):
        with pytest.raises(ValueError):
            PackedLayout(bad, 48)
    with pytest.raises(ValueError):
        lay.check(2, 64, torch.device("cpu"))
