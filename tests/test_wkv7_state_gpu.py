"""The WKV7 training op with a carried state on the MI355X: vrwkv_wkv7_backward_state_bf16 (variants 5 / 8 / 9), the autograd node and
the state-tuning model layer.  Reference and limits: tests/state_ref.py."""
from types import SimpleNamespace

import pytest
import torch

from oracle import wkv7_c
from oracle.wkv7_oracle import make_inputs, rel_rms
from tests.parity import bf16_close
from tests.state_ref import DS_TOL, FLIP_G, FLIP_W, FLIP_Y, NAMES, TOL, check_grads, reference, rel_rms64, state_inputs

pytestmark = pytest.mark.gpu


def _fwd(ins, s0):
    from visualrwkv_amd import wkv7
    B, T, H, _ = ins[0].shape
    s = torch.empty(B, H, T // 16, 64, 64, dtype=torch.float32, device=ins[0].device)
    sa = torch.empty(B, T, H, 64, dtype=torch.float32, device=ins[0].device)
    y, fin = wkv7.wkv7_forward_state(*ins, s0, want_state=True, s_ckpt=s, sa=sa)
    return y, fin, s, sa


@pytest.mark.parametrize("variant", [5, 8, 9])
@pytest.mark.parametrize("B,T,H", [(1, 16, 1), (2, 64, 3), (1, 384, 12), (3, 208, 5)])
def test_state_backward_against_fp64(hip_lib, B, T, H, variant):
    from visualrwkv_amd import wkv7
    ins, dy, s0, dsT = state_inputs(B, T, H, seed=B + T + H)
    yr, finr, gr, ds0r = reference(ins, dy, s0, dsT)
    d = [x.cuda() for x in ins]
    y, fin, s, sa = _fwd(d, s0.cuda())
    assert hip_lib.vrwkv_wkv7_set_backward_variant(variant) == 0
    try:
        *g, ds0 = wkv7.wkv7_backward_state(*d, dy.cuda(), s, sa, s0.cuda(), dsT.cuda(), True)
        torch.cuda.synchronize()
        assert hip_lib.vrwkv_wkv7_last_variant(1) == variant == hip_lib.vrwkv_wkv7_resolve_variant(3, B, T, H)
    finally:
        hip_lib.vrwkv_wkv7_set_backward_variant(-1)
    bf16_close(y, yr, "y", tol=TOL, max_flip=FLIP_Y)
    assert rel_rms64(fin.cpu(), finr) < 2e-5
    e = rel_rms64(ds0.cpu(), ds0r)
    print(f"[state] ({B},{T},{H}) variant {variant}: ds0 rel-RMS {e:.3e}")
    check_grads(g, gr, f"({B},{T},{H}) variant {variant}")
    assert e < DS_TOL, e


PAIRS = [(0, 0), (3, 17), (7, 31), (-1, 5)]        # the (b, h) sample the fp64 reference is computed for (b = -1: the last sample)


@pytest.mark.parametrize("B,T,H", [(16, 2624, 32), (8, 6400, 32)])
def test_state_backward_default_dispatch_at_bench_shapes(hip_lib, B, T, H):
    """No variant forced; the fp64 reference for four (b, h) pairs only, each as a (1, T, 1, 64) problem (heads and samples are independent)."""
    from visualrwkv_amd import wkv7
    assert hip_lib.vrwkv_wkv7_set_backward_variant(-1) == 0
    ins, dy, s0, dsT = state_inputs(B, T, H, seed=B + T)
    d = [x.cuda() for x in ins]
    y, fin, s, sa = _fwd(d, s0.cuda())
    *g, ds0 = wkv7.wkv7_backward_state(*d, dy.cuda(), s, sa, s0.cuda(), dsT.cuda(), True)
    torch.cuda.synchronize()
    want = hip_lib.vrwkv_wkv7_resolve_variant(3, B, T, H)
    assert hip_lib.vrwkv_wkv7_last_variant(1) == want == (9 if B * H > 256 else 8)
    del s, sa
    g = [x.cpu() for x in g]
    ds0, y = ds0.cpu(), y.cpu()
    for b, h in PAIRS:
        one = [x[b:b + 1 if b >= 0 else None, :, h:h + 1][-1:].contiguous() for x in ins]
        sl = lambda x: x[b, :, h].unsqueeze(0).unsqueeze(2)
        yr, _, gr, ds0r = reference(one, sl(dy), s0[b, h][None, None], dsT[b, h][None, None])
        bf16_close(sl(y), yr, f"y ({b},{h})", tol=TOL, max_flip=FLIP_Y)
        check_grads([sl(x) for x in g], gr, f"({B},{T},{H}) pair ({b},{h})")
        e = rel_rms64(ds0[b, h], ds0r[0, 0])
        print(f"[state] ({B},{T},{H}) pair ({b},{h}): ds0 rel-RMS {e:.3e}")
        assert e < DS_TOL, e


def test_null_pointers_are_the_plain_backward(hip_lib):
    from visualrwkv_amd import wkv7
    B, T, H = 16, 2624, 32
    w, q, k, v, z, a, dy = [x.cuda() for x in make_inputs(B, T, H, seed=5)]
    _, _, s, sa = _fwd([w, q, k, v, z, a], None)
    ref = [torch.empty_like(w) for _ in range(6)]
    torch.ops.wind_backstepping.backward(w, q, k, v, z, a, dy, s, sa, *ref)
    *g, ds0 = wkv7.wkv7_backward_state(w, q, k, v, z, a, dy, s, sa, None, None, False)
    torch.cuda.synchronize()
    assert ds0 is None and hip_lib.vrwkv_wkv7_last_variant(1) == 9
    for n, a_, b_ in zip(NAMES, g, ref):
        assert torch.equal(a_, b_), n


def test_split_identity_at_the_bench_shape(hip_lib):
    """(16, 2624, 32) cut at 1312, zero state0, no dL/dS_T: the two parts chained through the state at the cut and its gradient against the
    C oracle's whole-sequence backward -- every head's state-gradient path at scale, without an fp64 run."""
    from visualrwkv_amd import wkv7
    B, T, H, cut = 16, 2624, 32, 1312
    w, q, k, v, z, a, dy = make_inputs(B, T, H, seed=B + T)
    yr, sr, sar = wkv7_c.forward(w, q, k, v, z, a)
    ref = wkv7_c.backward(w, q, k, v, z, a, dy, sr, sar)
    del sr, sar
    p1 = [x[:, :cut].contiguous().cuda() for x in (w, q, k, v, z, a)]
    p2 = [x[:, cut:].contiguous().cuda() for x in (w, q, k, v, z, a)]
    y1, mid, s1, sa1 = _fwd(p1, None)
    y2, _, s2, sa2 = _fwd(p2, mid)
    *g2, dmid = wkv7.wkv7_backward_state(*p2, dy[:, cut:].contiguous().cuda(), s2, sa2, mid, None, True)
    *g1, ds0 = wkv7.wkv7_backward_state(*p1, dy[:, :cut].contiguous().cuda(), s1, sa1, None, dmid, False)
    torch.cuda.synchronize()
    bf16_close(torch.cat([y1, y2], dim=1), yr.float(), "y", tol=TOL, max_flip=FLIP_Y)
    for n, a_, b_, r in zip(NAMES, g1, g2, ref):
        bf16_close(torch.cat([a_, b_], dim=1), r.float(), f"chained {n}", tol=TOL, max_flip=FLIP_W if n in ("dw", "dz") else FLIP_G)


@pytest.mark.parametrize("variant", [-1, 9])                # -1: schedule 8 at this size
def test_state_backward_batch_slices(hip_lib, variant):
    """The launcher slices s0 / ds_final / ds0 per sample with the batch (tensors of 4 GiB and more in production; the limit lowered here):
    3 samples as slices of 2 + 1 are bit-identical to one launch, a single sample above the limit goes to the 64-bit kernel (variant 5)."""
    from visualrwkv_amd import wkv7
    B, T, H = 3, 32, 2
    ins, dy, s0, dsT = state_inputs(B, T, H, seed=92 + variant)
    _, _, gr, ds0r = reference(ins, dy, s0, dsT)
    d, s0d = [x.cuda() for x in ins], s0.cuda()
    _, _, s, sa = _fwd(d, s0d)
    args = (*d, dy.cuda(), s, sa, s0d, dsT.cuda(), True)
    per_sample = T * H * 64 * 4
    assert hip_lib.vrwkv_wkv7_set_backward_variant(variant) == 0
    try:
        base = wkv7.wkv7_backward_state(*args)
        assert hip_lib.vrwkv_wkv7_set_backward_slice_limit(2 * per_sample + 1) == 0
        sliced = wkv7.wkv7_backward_state(*args)
        torch.cuda.synchronize()
        assert hip_lib.vrwkv_wkv7_last_variant(1) == (8 if variant == -1 else variant)
        for n, o, r in zip(NAMES + ("ds0",), sliced, base):
            assert torch.equal(o, r), n
        assert hip_lib.vrwkv_wkv7_set_backward_slice_limit(per_sample // 2) == 0
        *wide, wide_ds0 = wkv7.wkv7_backward_state(*args)
        torch.cuda.synchronize()
        assert hip_lib.vrwkv_wkv7_last_variant(1) == 5
    finally:
        hip_lib.vrwkv_wkv7_set_backward_slice_limit(0)
        hip_lib.vrwkv_wkv7_set_backward_variant(-1)
    check_grads(wide, gr, f"one sample above the limit, override {variant}")
    assert rel_rms64(wide_ds0.cpu(), ds0r) < DS_TOL


def _visual(grad_cp):
    from visualrwkv_amd.visual import VisualRWKV
    args = SimpleNamespace(n_embd=2048, n_layer=2, dim_att=2048, head_size_a=64, head_size_divisor=8, vocab_size=65536,
                           dropout=0, grad_cp=grad_cp, ctx_len=64, num_token_per_image=16, vision_towers=("dino",),
                           vision_image_size=56, load_model="", proj_type="mlp", weight_decay=0.0, fused=True, state_tune=1,
                           vision_tower_kwargs={"dino": dict(depth=1, dim=64, heads=1)})
    torch.manual_seed(0)
    m = VisualRWKV(args)
    with torch.no_grad():
        for b in m.rwkv.blocks:
            b.att.output.weight.normal_(0, 0.02)
            b.ffn.value.weight.normal_(0, 0.02)
            b.att.time_state.normal_(0, 0.1)
    return m.bfloat16().cuda()


def test_state_tuning_step_under_every_memory_mode():
    """training_step of a 2-layer C = 2048 model with state_tune: loss and time_state gradients under grad_cp 0, 1, 2 agree to the bounds
    tests/test_model_gpu.py::test_selective_recompute_keeps_less_and_computes_the_same holds the stateless model's modes to (2e-3 on the
    output, 4e-3 on gradients); nothing else gets a gradient."""
    m = _visual(0)
    m.freeze_for_state_tuning()
    g = torch.Generator(device="cuda").manual_seed(1)
    ids = torch.randint(0, 1000, (2, 64), device="cuda", generator=g)
    labels = ids.clone(); labels[:, :8] = -100
    batch = {"input_ids": ids, "labels": labels, "sample_id": ["0", "1"]}
    res = {}
    for mode in (0, 1, 2):
        m.args.grad_cp = mode
        m.zero_grad(set_to_none=True)
        loss = m.training_step(batch)
        loss.backward()
        grads = {}
        for n, p in m.named_parameters():
            if n.endswith(".time_state"):
                assert p.grad is not None and p.grad.dtype == torch.bfloat16 and float(p.grad.float().abs().max()) > 0, n
                grads[n] = p.grad.float().cpu()
            else:
                assert p.grad is None, n
        res[mode] = (float(loss.detach()), grads)
    assert len(res[0][1]) == 2
    for mode in (1, 2):
        assert abs(res[mode][0] - res[0][0]) < 2e-3 * abs(res[0][0]), (mode, res[mode][0], res[0][0])
        for n, gr in res[0][1].items():
            assert rel_rms(res[mode][1][n], gr) < 4e-3, (mode, n)


def test_generation_starts_from_the_tuned_state():
    from visualrwkv_amd.rwkv7 import IMAGE_TOKEN_INDEX
    m = _visual(0).eval()
    ids = torch.randint(0, 256, (1, 32), device="cuda")
    x = m.rwkv.emb(ids)
    with torch.no_grad():
        full = m.rwkv(x)
        got, state = m.rwkv.forward_stateful(x, None)
        assert torch.equal(got.argmax(-1), full.argmax(-1))
        assert rel_rms(got.float(), full.float()) < 2e-2        # the bound of tests/test_stateful_gpu.py::test_model_stateful_equals_full_forward
        keep = [b.att.time_state.detach().clone() for b in m.rwkv.blocks]
        for b in m.rwkv.blocks:                                  # the state matters: from zeros the logits move
            b.att.time_state.zero_()
        assert rel_rms(m.rwkv(x).float(), full.float()) > 1e-2
        for b, t in zip(m.rwkv.blocks, keep):
            b.att.time_state.copy_(t)
    ids[0, 3:19] = IMAGE_TOKEN_INDEX
    images = {"dino": torch.randn(1, 3, 56, 56, device="cuda", dtype=torch.bfloat16)}
    ref = m.generate(ids, images, False, 1.0, 1.0, 1, stop_token_idx=-7)
    out = m.generate_stateful(ids, images, False, 1.0, 1.0, 8, stop_token_idx=-7)       # 8 tokens: the captured decode step, from the tuned state
    assert len(out[0]) == 8 and out[0][0] == ref[0][0]
