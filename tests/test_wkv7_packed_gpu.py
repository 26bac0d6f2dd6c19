"""Packed rows on the MI355X: vrwkv_wkv7_forward_packed_bf16 / vrwkv_wkv7_backward_packed_bf16 (csrc/wkv7_fwd_v4.h and the schedules 8 / 9 of
csrc/wkv7_bwd_v8.h with resets at sample boundaries) and the autograd node.  Reference: fp64 autograd through the oracle recurrence on every
segment's slice alone, concatenated; limits: tests/state_ref.py.  And bit-identity against the plain entries launched per segment.

About dw: dL/dw of a sample's first token is exactly 0 (w of that token multiplies the zero state before it; the fp64 reference has 0.0).
The packed backward writes that 0 at the first token of a flagged chunk; the plain kernel, which cannot know that a launch starts from zero,
leaves the cancellation residue of its sum there (~5e-5 against |dw| ~ 0.3), and bf16_close would count every such element as a flip.  So
dw is bit-identical to the per-segment launches on every token but a segment's first, exactly 0 there, and held to the fp64 limits as a
whole; everything else is bit-identical throughout (tests/test_emulated_wkv7_packed.py says the same of the emulated kernels)."""
import random

import pytest
import torch

from oracle.wkv7_oracle import make_inputs
from tests.parity import bf16_close
from tests.state_ref import FLIP_Y, NAMES, TOL, check_grads, reference
from tests.test_wkv7_state_gpu import PAIRS

pytestmark = pytest.mark.gpu


def _segments(row):
    t, out = 0, []
    for n in row:
        out.append((t, t + n))
        t += n
    return out


def _few_samples_layout(B, T, seed):
    """Two or three samples per row, cut at random chunk boundaries: what a packer makes of a handful of conversations."""
    rng = random.Random(seed)
    rows = []
    for _ in range(B):
        cuts = sorted(rng.sample(range(1, T // 16), rng.randint(1, 2)))
        rows.append([16 * (b - a) for a, b in zip([0] + cuts, cuts + [T // 16])])
    return rows


def _bench_layout(B, T, seed):
    """Segment lengths 16 * U{1..60}; the last segment of a row takes the rest."""
    rng = random.Random(seed)
    rows = []
    for _ in range(B):
        row, left = [], T
        while left > 0:
            n = min(16 * rng.randint(1, 60), left)
            row.append(n)
            left -= n
        rows.append(row)
    return rows


def _run_packed(d, dy, lay):
    from visualrwkv_amd import wkv7
    B, T, H, _ = d[0].shape
    s = torch.empty(B, H, T // 16, 64, 64, dtype=torch.float32, device="cuda")
    sa = torch.empty(B, T, H, 64, dtype=torch.float32, device="cuda")
    y = wkv7.wkv7_forward_packed(*d, lay, s_ckpt=s, sa=sa)
    g = wkv7.wkv7_backward_packed(*d, dy, s, sa, lay)
    torch.cuda.synchronize()
    return y, s, sa, list(g)


def _reference_rows(ins, dy, rows, sel=None):
    """fp64 per segment, concatenated.  sel = (b, h): that row and head only, as (1, T, 1, 64) problems."""
    pick = (lambda x: x) if sel is None else (lambda x: x[sel[0], :, sel[1]].unsqueeze(0).unsqueeze(2))
    ins, dy = [pick(x) for x in ins], pick(dy)
    rows = rows if sel is None else [rows[sel[0]]]
    yr = torch.zeros(ins[0].shape, dtype=torch.float64)
    gr = [torch.zeros(ins[0].shape, dtype=torch.float64) for _ in range(6)]
    for b, row in enumerate(rows):
        for t0, t1 in _segments(row):
            y1, _, g1, _ = reference([x[b:b + 1, t0:t1].contiguous() for x in ins], dy[b:b + 1, t0:t1].contiguous())
            yr[b:b + 1, t0:t1] = y1
            for a_, b_ in zip(gr, g1):
                a_[b:b + 1, t0:t1] = b_
    return yr, gr


def _figures(x, ref):
    xr, rr = x.float().cpu().reshape(-1), ref.double().reshape(-1).float().bfloat16().float()
    return float((xr - rr).double().norm() / rr.double().norm().clamp_min(1e-30)), float((xr != rr).float().mean())


def _print_dw(what, dw, dwr, first):
    print(f"[packed] {what} dw: rel-RMS %.3e flips %.4f" % _figures(dw, dwr), "| without first tokens: rel-RMS %.3e flips %.4f" % _figures(dw.cpu()[~first], dwr[~first]))


@pytest.mark.parametrize("variant", [8, 9])
@pytest.mark.parametrize("B,T,H", [(2, 160, 2), (3, 208, 5), (1, 384, 12)])
def test_packed_small_shapes(hip_lib, B, T, H, variant):
    """Bit-identity against the plain entries per segment with the same kernels forced, then the fp64 limits on the whole packed tensors.
    The forward override is 7 for the sake of the PLAIN per-segment launches: the packed forward runs wkv7_fwd_v4.h whatever it says
    (test_packed_forward_ignores_the_forward_override), while the plain op at these sizes would pick wkv7_fwd_v3.h, another summation order."""
    from visualrwkv_amd import wkv7
    rows = _few_samples_layout(B, T, seed=B + T + H)
    *ins, dy = make_inputs(B, T, H, seed=B + T + H + variant)
    lay = wkv7.PackedLayout(rows, T, "cuda")
    d, dyd = [x.cuda() for x in ins], dy.cuda()
    assert hip_lib.vrwkv_wkv7_set_backward_variant(variant) == 0 and hip_lib.vrwkv_wkv7_set_forward_variant(7) == 0
    try:
        assert hip_lib.vrwkv_wkv7_resolve_variant(4, B, T, H) == 7 and hip_lib.vrwkv_wkv7_resolve_variant(5, B, T, H) == variant
        y, s, sa, g = _run_packed(d, dyd, lay)
        assert hip_lib.vrwkv_wkv7_last_variant(0) == 7 and hip_lib.vrwkv_wkv7_last_variant(1) == variant
        # the plain entries on every segment alone, same kernels forced
        for b, row in enumerate(rows):
            for t0, t1 in _segments(row):
                cut = [x[b:b + 1, t0:t1].contiguous() for x in d]
                n = t1 - t0
                y1 = torch.empty_like(cut[0])
                s1 = torch.empty(1, H, n // 16, 64, 64, dtype=torch.float32, device="cuda")
                sa1 = torch.empty(1, n, H, 64, dtype=torch.float32, device="cuda")
                torch.ops.wind_backstepping.forward(*cut, y1, s1, sa1)
                g1 = [torch.empty_like(cut[0]) for _ in range(6)]
                torch.ops.wind_backstepping.backward(*cut, dyd[b:b + 1, t0:t1].contiguous(), s1, sa1, *g1)
                torch.cuda.synchronize()
                assert hip_lib.vrwkv_wkv7_last_variant(0) == 7 and hip_lib.vrwkv_wkv7_last_variant(1) == variant
                what = f"({B},{T},{H}) variant {variant} row {b} tokens {t0}:{t1}"
                assert torch.equal(y[b:b + 1, t0:t1], y1), f"{what} y"
                assert torch.equal(sa[b:b + 1, t0:t1], sa1), f"{what} sa"
                assert torch.equal(s[b:b + 1, :, t0 // 16:t1 // 16], s1), f"{what} s_ckpt"
                for nm, a_, b_ in zip(NAMES, g, g1):
                    skip = 1 if nm == "dw" else 0                  # the first token's dw: exact 0 here, a residue there (module docstring)
                    assert torch.equal(a_[b:b + 1, t0 + skip:t1], b_[:, skip:]), f"{what} {nm}"
                assert float(g[0][b, t0].float().abs().max()) == 0.0, f"{what} dw of the first token"
    finally:
        hip_lib.vrwkv_wkv7_set_backward_variant(-1)
        hip_lib.vrwkv_wkv7_set_forward_variant(-1)
    yr, gr = _reference_rows(ins, dy, rows)
    _print_dw(f"({B},{T},{H}) variant {variant}", g[0], gr[0], lay.first.view(B, T).bool().cpu())
    bf16_close(y, yr, "y", tol=TOL, max_flip=FLIP_Y)
    check_grads(g, gr, f"({B},{T},{H}) variant {variant}")


@pytest.mark.parametrize("forced", [-1, 4, 6, 7])
def test_packed_forward_ignores_the_forward_override(hip_lib, forced):
    """Default dispatch (-1; the plain op would run two workgroups per head here) and any override: kind 4 resolves to 7 and y, s, sa are the same bits."""
    from visualrwkv_amd import wkv7
    B, T, H = 2, 160, 2
    rows = _few_samples_layout(B, T, seed=1)
    *ins, dy = make_inputs(B, T, H, seed=2)
    lay = wkv7.PackedLayout(rows, T, "cuda")
    d = [x.cuda() for x in ins]
    assert hip_lib.vrwkv_wkv7_set_forward_variant(7) == 0
    try:
        ref = _run_packed(d, dy.cuda(), lay)
        assert hip_lib.vrwkv_wkv7_set_forward_variant(forced) == 0
        assert hip_lib.vrwkv_wkv7_resolve_variant(4, B, T, H) == 7
        got = _run_packed(d, dy.cuda(), lay)
        assert hip_lib.vrwkv_wkv7_last_variant(0) == 7
    finally:
        hip_lib.vrwkv_wkv7_set_forward_variant(-1)
    assert all(torch.equal(a_, b_) for a_, b_ in zip(ref[:3], got[:3]))


@pytest.mark.parametrize("B,T,H", [(16, 2624, 32), (8, 6400, 32)])
def test_packed_default_dispatch_at_bench_shapes(hip_lib, B, T, H):
    """No variant forced; the per-segment fp64 reference for four (b, h) pairs, each segment a (1, len, 1, 64) problem."""
    from visualrwkv_amd import wkv7
    assert hip_lib.vrwkv_wkv7_set_backward_variant(-1) == 0 and hip_lib.vrwkv_wkv7_set_forward_variant(-1) == 0
    rows = _bench_layout(B, T, seed=B + T)
    *ins, dy = make_inputs(B, T, H, seed=B + T)
    lay = wkv7.PackedLayout(rows, T, "cuda")
    y, s, sa, g = _run_packed([x.cuda() for x in ins], dy.cuda(), lay)
    want = 9 if B * H > 256 else 8
    assert hip_lib.vrwkv_wkv7_resolve_variant(4, B, T, H) == 7 == hip_lib.vrwkv_wkv7_last_variant(0)
    assert hip_lib.vrwkv_wkv7_resolve_variant(5, B, T, H) == want == hip_lib.vrwkv_wkv7_last_variant(1) == hip_lib.vrwkv_wkv7_resolve_variant(1, B, T, H)
    del s, sa
    y, g = y.cpu(), [x.cpu() for x in g]
    first = lay.first.view(B, T).bool().cpu()
    for b, h in PAIRS:
        b = b % B
        sl = lambda x: x[b, :, h].unsqueeze(0).unsqueeze(2)
        yr, gr = _reference_rows(ins, dy, rows, sel=(b, h))
        _print_dw(f"({B},{T},{H}) pair ({b},{h}), {len(rows[b])} segments", sl(g[0]), gr[0], first[b].view(1, T))
        bf16_close(sl(y), yr, f"y ({b},{h})", tol=TOL, max_flip=FLIP_Y)
        check_grads([sl(x) for x in g], gr, f"({B},{T},{H}) pair ({b},{h})")


@pytest.mark.parametrize("null", [False, True])
@pytest.mark.parametrize("B,T,H", [(16, 2624, 32), (8, 6400, 32)])
def test_no_resets_is_the_plain_op(hip_lib, B, T, H, null):
    from visualrwkv_amd import wkv7
    w, q, k, v, z, a, dy = [x.cuda() for x in make_inputs(B, T, H, seed=5)]
    y0 = torch.empty_like(v)
    s0 = torch.empty(B, H, T // 16, 64, 64, dtype=torch.float32, device="cuda")
    sa0 = torch.empty(B, T, H, 64, dtype=torch.float32, device="cuda")
    torch.ops.wind_backstepping.forward(w, q, k, v, z, a, y0, s0, sa0)
    ref = [torch.empty_like(w) for _ in range(6)]
    torch.ops.wind_backstepping.backward(w, q, k, v, z, a, dy, s0, sa0, *ref)
    lay = wkv7.PackedLayout([[T]] * B, T, "cuda")
    assert int(lay.chunk_reset[:, 1:].sum()) == 0
    lay.chunk_reset.zero_()                                  # chunk 0 starts from S = 0 with or without its flag
    if null:
        lay.chunk_reset = torch.empty(0, dtype=torch.uint8, device="cuda")       # data_ptr() == 0: the NULL form of the entries
        assert lay.chunk_reset.data_ptr() == 0
    y, s, sa, g = _run_packed([w, q, k, v, z, a], dy, lay)
    assert torch.equal(y, y0) and torch.equal(s, s0) and torch.equal(sa, sa0)
    for n, a_, b_ in zip(NAMES, g, ref):
        assert torch.equal(a_, b_), n


@pytest.mark.parametrize("recompute", [False, True])
def test_autograd_node(hip_lib, recompute):
    from visualrwkv_amd import wkv7
    B, T, H = 3, 208, 5
    rows = _few_samples_layout(B, T, seed=11)
    *ins, dy = make_inputs(B, T, H, seed=12)
    yr, gr = _reference_rows(ins, dy, rows)
    lay = wkv7.PackedLayout(rows, T, "cuda")
    views = [x.cuda().view(B, T, H * 64).requires_grad_(True) for x in (ins[1], ins[0], *ins[2:])]       # (q, w, k, v, a, b) order
    y = wkv7.RUN_CUDA_RWKV7g_packed(*views, lay, recompute)
    (y.float() * dy.cuda().view(B, T, H * 64).float()).sum().backward()
    bf16_close(y.view(B, T, H, 64), yr, "y", tol=TOL, max_flip=FLIP_Y)
    got = [views[1].grad, views[0].grad, *[x.grad for x in views[2:]]]
    check_grads([x.view(B, T, H, 64) for x in got], gr, f"autograd node recompute {recompute}")
    with torch.no_grad():
        assert torch.equal(wkv7.RUN_CUDA_RWKV7g_packed(*views, lay), y)          # the entry without by-products


def test_override_5_runs_the_plain_op_per_segment(hip_lib):
    from visualrwkv_amd import wkv7
    B, T, H = 2, 160, 2
    rows = _few_samples_layout(B, T, seed=3)
    *ins, dy = make_inputs(B, T, H, seed=4)
    lay = wkv7.PackedLayout(rows, T, "cuda")
    d, dyd = [x.cuda() for x in ins], dy.cuda()
    y, s, sa, g = _run_packed(d, dyd, lay)
    assert hip_lib.vrwkv_wkv7_set_backward_variant(5) == 0
    try:
        g5 = wkv7.wkv7_backward_packed(*d, dyd, s, sa, lay)
        torch.cuda.synchronize()
    finally:
        hip_lib.vrwkv_wkv7_set_backward_variant(-1)
    _, gr = _reference_rows(ins, dy, rows)
    check_grads(list(g5), gr, "override 5, per segment")


@pytest.mark.parametrize("variant", [8, 9])
def test_packed_backward_batch_slices(hip_lib, variant):
    """The launcher slices chunk_reset per row with the batch (the limit lowered here): 3 rows, another reset pattern in each, as slices of
    2 + 1 are bit-identical to one launch."""
    from visualrwkv_amd import wkv7
    B, T, H = 3, 32, 2
    rows = [[32], [16, 16], [32]]
    *ins, dy = make_inputs(B, T, H, seed=93 + variant)
    lay = wkv7.PackedLayout(rows, T, "cuda")
    lay.chunk_reset.copy_(torch.tensor([[1, 0], [1, 1], [0, 1]], dtype=torch.uint8))       # resets at chunks {0}, {0, 1}, {1}
    d, dyd = [x.cuda() for x in ins], dy.cuda()
    per_sample = T * H * 64 * 4
    assert hip_lib.vrwkv_wkv7_set_backward_variant(variant) == 0
    try:
        _, s, sa, base = _run_packed(d, dyd, lay)
        assert hip_lib.vrwkv_wkv7_last_variant(1) == variant
        assert hip_lib.vrwkv_wkv7_set_backward_slice_limit(2 * per_sample + 1) == 0
        sliced = wkv7.wkv7_backward_packed(*d, dyd, s, sa, lay)
        torch.cuda.synchronize()
        assert hip_lib.vrwkv_wkv7_last_variant(1) == variant
        for n, o, r in zip(NAMES, sliced, base):
            assert torch.equal(o, r), n
    finally:
        hip_lib.vrwkv_wkv7_set_backward_slice_limit(0)
        hip_lib.vrwkv_wkv7_set_backward_variant(-1)
