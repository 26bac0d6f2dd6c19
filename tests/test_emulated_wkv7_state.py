"""The WKV7 training backward with a carried state on the host lockstep emulator: the STATE instantiations of
csrc/wkv7_bwd_v8.h (schedules 8 and 9), the C entry vrwkv_wkv7_backward_state_bf16 and the autograd node on top of it,
against fp64 autograd through the oracle recurrence (tests/state_ref.py)."""
import contextlib
import ctypes

import pytest
import torch

from tests.state_ref import DS_TOL, NAMES, P, check_grads, reference, rel_rms64, state_inputs
from tests.parity import bf16_close
from tests.state_ref import FLIP_Y, TOL


def _forward(emu, ins, s0):
    B, T, H, _ = ins[0].shape
    y = torch.zeros_like(ins[3])
    s, sa, fin = torch.zeros(B, H, T // 16, 64, 64), torch.zeros(B, T, H, 64), torch.zeros(B, H, 64, 64)
    emu.emu_wkv7_forward_state_train(B, T, H, *[P(x) for x in ins], P(y), P(s0), P(fin), P(s), P(sa))
    return y, fin, s, sa


def _backward(emu, ins, dy, s, sa, s0, ds_in, want_ds0, ahead):
    B, T, H, _ = ins[0].shape
    g = [torch.zeros_like(ins[0]) for _ in range(6)]
    ds0 = torch.zeros(B, H, 64, 64) if want_ds0 else None
    emu.emu_wkv7_backward_state_v8(B, T, H, *[P(x) for x in ins], P(dy), P(s), P(sa), P(s0), P(ds_in), P(ds0), *[P(x) for x in g], ahead)
    return g, ds0


@pytest.mark.parametrize("ahead", [0, 1])
@pytest.mark.parametrize("T", [16, 32, 48, 80, 160])
def test_state_kernel_against_fp64(emu_lib, T, ahead):
    """1, 2, 3, 5 and 10 chunks (pipeline shorter than, equal to and longer than its depth), random state0 and dL/dS_T."""
    B, H = 1, 2
    ins, dy, s0, dsT = state_inputs(B, T, H, seed=T + ahead)
    y, fin, s, sa = _forward(emu_lib, ins, s0)
    yr, finr, gr, ds0r = reference(ins, dy, s0, dsT)
    bf16_close(y, yr, "y", tol=TOL, max_flip=FLIP_Y)
    g, ds0 = _backward(emu_lib, ins, dy, s, sa, s0, dsT, True, ahead)
    check_grads(g, gr, f"state T={T} schedule {8 + ahead}")
    e = rel_rms64(ds0, ds0r)
    print(f"[state] T={T} schedule {8 + ahead}: ds0 rel-RMS {e:.3e}")
    assert e < DS_TOL, e


@pytest.mark.parametrize("ahead", [0, 1])
@pytest.mark.parametrize("T", [16, 48, 160])
def test_null_state_pointers_are_the_plain_kernel(emu_lib, T, ahead):
    B, H = 1, 2
    ins, dy, _, _ = state_inputs(B, T, H, seed=3 * T + ahead)
    _, _, s, sa = _forward(emu_lib, ins, None)
    g, _ = _backward(emu_lib, ins, dy, s, sa, None, None, False, ahead)
    ref = [torch.zeros_like(ins[0]) for _ in range(6)]
    emu_lib.emu_wkv7_backward_chunked(B, T, H, *[P(x) for x in ins], P(dy), P(s), P(sa), *[P(x) for x in ref], 9 + ahead)
    for n, a_, b_ in zip(NAMES, g, ref):
        assert torch.equal(a_, b_), n


@pytest.mark.parametrize("ahead", [0, 1])
def test_split_identity(emu_lib, ahead):
    """T = 160 cut at 64: forward and backward of the two parts chained through the state at the cut and its gradient reproduce the
    one-launch results."""
    B, T, H, cut = 1, 160, 2, 64
    ins, dy, s0, dsT = state_inputs(B, T, H, seed=77 + ahead)
    _, _, gr, ds0r = reference(ins, dy, s0, dsT)
    _, _, s, sa = _forward(emu_lib, ins, s0)
    g_whole, ds0_whole = _backward(emu_lib, ins, dy, s, sa, s0, dsT, True, ahead)
    p1 = [x[:, :cut].contiguous() for x in ins]
    p2 = [x[:, cut:].contiguous() for x in ins]
    _, mid, s1, sa1 = _forward(emu_lib, p1, s0)
    _, fin, s2, sa2 = _forward(emu_lib, p2, mid)
    g2, dmid = _backward(emu_lib, p2, dy[:, cut:].contiguous(), s2, sa2, mid, dsT, True, ahead)
    g1, ds0 = _backward(emu_lib, p1, dy[:, :cut].contiguous(), s1, sa1, s0, dmid, True, ahead)
    got = [torch.cat([a_, b_], dim=1) for a_, b_ in zip(g1, g2)]
    check_grads(got, gr, "chained parts vs fp64")
    check_grads(got, [x.double() for x in g_whole], "chained parts vs one launch")
    e, ew = rel_rms64(ds0, ds0r), rel_rms64(ds0, ds0_whole)
    print(f"[state] split schedule {8 + ahead}: ds0 rel-RMS {e:.3e} vs fp64, {ew:.3e} vs one launch")
    assert e < DS_TOL and ew < DS_TOL


def _shim(emu):
    V = lambda p: ctypes.c_void_p(p) if p else None

    class Shim:
        @staticmethod
        def vrwkv_wkv7_forward_state_bf16(B, T, H, w, q, k, v, z, a, y, s0, s_fin, s_ckpt, sa, stream):
            return emu.emu_wkv7_forward_state_train(B, T, H, V(w), V(q), V(k), V(v), V(z), V(a), V(y), V(s0), V(s_fin), V(s_ckpt), V(sa))

        @staticmethod
        def vrwkv_wkv7_backward_state_bf16(B, T, H, *rest):
            fn = emu.vrwkv_wkv7_backward_state_bf16                 # csrc/wkv7_capi.hip itself, compiled for the host
            fn.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 19
            return fn(B, T, H, *[V(p) for p in rest])

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


@pytest.mark.parametrize("variant", [-1, 5, 9])           # -1: schedule 8 at this size
@pytest.mark.parametrize("recompute", [False, True])
def test_autograd_node_through_the_c_entry(emu_lib, emulated_op, variant, recompute):
    B, T, H = 2, 48, 2
    ins, dy, s0, dsT = state_inputs(B, T, H, seed=11 + variant)
    yr, finr, gr, ds0r = reference(ins, dy, s0, dsT)
    leaves = [x.clone().requires_grad_(True) for x in ins]
    s0l = s0.clone().requires_grad_(True)
    assert emu_lib.vrwkv_wkv7_set_backward_variant(variant) == 0
    try:
        y, fin = emulated_op.WindBacksteppingState.apply(*leaves, s0l, recompute)
        ((y.float() * dy.float()).sum() + (fin * dsT).sum()).backward()
        assert emu_lib.vrwkv_wkv7_last_variant(1) == emu_lib.vrwkv_wkv7_resolve_variant(3, B, T, H) == (8 if variant == -1 else variant)
    finally:
        emu_lib.vrwkv_wkv7_set_backward_variant(-1)
    bf16_close(y, yr, "y", tol=TOL, max_flip=FLIP_Y)
    assert rel_rms64(fin, finr) < 2e-5                     # the bound tests/test_emulated_wkv7.py::test_forward_from_state holds the final state to
    check_grads([l.grad for l in leaves], gr, f"autograd node variant {variant}")
    e = rel_rms64(s0l.grad, ds0r)
    print(f"[state] autograd node variant {variant} recompute {recompute}: ds0 rel-RMS {e:.3e}")
    assert e < DS_TOL


def test_broadcast_state_unused_final_state_and_frozen_state(emulated_op):
    B, T, H = 2, 32, 2
    ins, dy, s0, _ = state_inputs(B, T, H, seed=5)
    s0 = s0[0].contiguous()                                  # (H,64,64): one state for every sample
    full = s0.unsqueeze(0).expand(B, H, 64, 64).contiguous()
    _, _, gr, ds0r = reference(ins, dy, full, None)
    views = [x.view(B, T, H * 64).clone().requires_grad_(True) for x in (ins[1], ins[0], *ins[2:])]       # (q, w, k, v, a, b) order
    s0l = s0.clone().requires_grad_(True)
    y, _ = emulated_op.RUN_CUDA_RWKV7g_state(*views, s0l)      # state_T unused: the backward gets no gradient for it (NULL ds_final)
    (y.float() * dy.view(B, T, H * 64).float()).sum().backward()
    got = [views[1].grad, views[0].grad, *[x.grad for x in views[2:]]]
    check_grads([x.view(B, T, H, 64) for x in got], gr, "broadcast state")
    assert s0l.grad.shape == s0.shape and s0l.grad.dtype == torch.float32
    assert rel_rms64(s0l.grad, ds0r.sum(0)) < DS_TOL        # gradient of a broadcast state = the sum over the batch
    # state0 without requires_grad: NULL ds0, same gradients
    views2 = [x.detach().clone().requires_grad_(True) for x in views]
    y2, _ = emulated_op.RUN_CUDA_RWKV7g_state(*views2, s0)
    (y2.float() * dy.view(B, T, H * 64).float()).sum().backward()
    for a_, b_ in zip(views, views2):
        assert torch.equal(a_.grad, b_.grad)
