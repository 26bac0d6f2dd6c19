"""VisualRWKV.train_step_cut under a single-process ZeRO-1 engine on the MI355X (collectives off), fused path: the K backward calls of a cut
step go through fused._weight_grad's flat-buffer path -- the first call's weight-gradient GEMM writes the weight's slot of the engine's flat
buffer and autograd adopts that view as `.grad`; later calls find `.grad` set, return a fresh tensor and autograd adds it in place -- inside
Zero1Engine.hold_reductions().  Held against the same cut step without an engine: the same kernels on the same values in the same order,
so the gradients are expected to be the same bits; asserted to the 4e-3 rel-RMS tests/test_packed_model_gpu.py holds two routes through
the same bf16 math to, the measured figure is printed."""
import pytest
import torch

from oracle.wkv7_oracle import rel_rms
from tests.test_cut_model_gpu import _batch, _visual

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("grad_cp", [0, 1])
def test_engine_cut_step_equals_the_cut_step_without_an_engine(grad_cp, monkeypatch):
    from visualrwkv_amd import fused
    from visualrwkv_amd.dp import Zero1Engine
    batch = _batch("cuda")
    m = _visual(grad_cp).bfloat16().cuda()
    m.zero_grad(set_to_none=True)
    loss_ref = float(m.train_step_cut(batch, 32))
    ref = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    eng = Zero1Engine(m, lr=1e-4, grad_clip=1.0, bucket_mb=20.0)
    assert not eng.collective and len(eng.buckets) > 2
    slot_writes, real = [], fused._weight_grad

    def counted(wp, dy2, x2):
        dw = real(wp, dy2, x2)
        if wp is not None and dw.data_ptr() == wp._vrwkv_flat_grad[0].data_ptr() + wp._vrwkv_flat_grad[1] * dw.element_size():
            slot_writes.append(id(wp))
        return dw
    monkeypatch.setattr(fused, "_weight_grad", counted)
    launched, real_launch = [], eng._launch_reduce
    eng._launch_reduce = lambda b: (launched.append(eng.buckets.index(b)), real_launch(b))[1]
    eng.zero_grad()
    loss = float(m.train_step_cut(batch, 32))
    # every Linear weight's slot was written by a GEMM exactly once (the first of the K = 4 backward calls), never again
    assert len(slot_writes) == len(set(slot_writes)) and len(slot_writes) >= 2 * 6 + 1, len(slot_writes)
    assert all(not getattr(p, "_vrwkv_wgrad_pending", False) for p in eng.params)
    assert launched == sorted(set(launched))                         # nothing reduced twice, index order
    eng.step()                                                       # flushes what is left; .grad are views of the flat buffer again
    assert sorted(launched) == list(range(len(eng.buckets)))
    assert loss == loss_ref
    worst = 0.0
    for n, p in m.named_parameters():
        if n in ref and ref[n].abs().max() > 0:
            assert p.grad.data_ptr() >= eng.flat_grad.data_ptr()
            e = rel_rms(p.grad.float(), ref[n].float())
            worst = max(worst, e)
            assert e < 4e-3, (n, e)
    print(f"[cut] engine against no engine, grad_cp {grad_cp}: worst gradient group rel-RMS {worst:.2e}")
    eng.close()
