"""Training a long row in segments on the MI355X: VisualRWKV.train_step_cut of the 2-layer C = 2048 model of tests/test_packed_model_gpu.py on
a (2, 128) batch cut at 64 and at 32, through the fused path -- fused.blocks_forward with a carry (the _carry token-shift kernels, the WKV7
state op) under its three memory modes, and the head on the labelled rows of every window (fused.HeadPlan with a window)."""
from types import SimpleNamespace

import pytest
import torch

from oracle.wkv7_oracle import rel_rms
from tests.parity import group_bias

pytestmark = pytest.mark.gpu

T = 128


def _visual(grad_cp, fused=True, **kw):
    """tests/test_packed_model_gpu.py::_visual."""
    from visualrwkv_amd.visual import VisualRWKV
    d = dict(n_embd=2048, n_layer=2, dim_att=2048, head_size_a=64, head_size_divisor=8, vocab_size=65536,
             dropout=0, grad_cp=grad_cp, ctx_len=T, num_token_per_image=16, vision_towers=("dino",),
             vision_image_size=56, load_model="", proj_type="mlp", weight_decay=0.0, fused=fused,
             check_image_tokens=not fused, vision_tower_kwargs={"dino": dict(depth=1, dim=64, heads=1)})
    d.update(kw)
    torch.manual_seed(0)
    m = VisualRWKV(SimpleNamespace(**d))
    with torch.no_grad():
        for b in m.rwkv.blocks:
            b.att.output.weight.normal_(0, 0.02)
            b.ffn.value.weight.normal_(0, 0.02)
    m.freeze_emb()
    return m


def _batch(device, t=T, image=True):
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, 1000, (2, t), generator=g)
    labels = ids.clone()
    labels[0, :4] = -100
    labels[1, :40] = -100                                   # a long prompt: unequal label counts per segment
    labels[:, 65:97] = -100                                 # rows 64 .. 95 predict tokens 65 .. 96: a 32-token segment without a label
    batch = {"input_ids": ids, "labels": labels, "sample_id": ["0", "1"]}
    if image:
        ids[0, 56:72] = 65535                               # a 16-token image span across the cut at 64
        labels[ids == 65535] = -100
        batch["images"] = {"dino": torch.randn(1, 3, 56, 56, generator=g).bfloat16().to(device)}
    batch["input_ids"], batch["labels"] = ids.to(device), labels.to(device)
    return batch


def _grads(m):
    return {n: p.grad.float().cpu() for n, p in m.named_parameters() if p.grad is not None}


def _uncut(m, batch):
    m.zero_grad(set_to_none=True)
    loss = m.training_step(batch)
    loss.backward()
    return float(loss.detach()), _grads(m)


def _cut(m, batch, seg_len):
    m.zero_grad(set_to_none=True)
    loss = m.train_step_cut(batch, seg_len)
    return float(loss), _grads(m)


def test_cut_step_under_every_memory_mode_and_against_fp32_cpu(monkeypatch):
    """The step takes fused.blocks_forward with a carry and fused.head_loss in every mode (counted: K - 1 segments forward without a graph,
    K with one, K windows of the head).  Every cut step is held against an fp32 CPU evaluation of the UNCUT batch to the bounds of
    tests/test_model_gpu.py::test_full_visual_step_matches_an_independent_fp32_cpu_evaluation (1e-2 on the loss; every gradient group
    2.6e-2 rel-RMS, scale error of the larger groups 8e-3).  Cut against uncut on the GPU is printed, not asserted: `.grad` accumulates in
    bf16 over the K backward calls."""
    from visualrwkv_amd import fused
    m = _visual(0).bfloat16().cuda()
    batch = _batch("cuda")
    seen = []
    real_blocks, real_head = fused.blocks_forward, fused.head_loss
    monkeypatch.setattr(fused, "blocks_forward", lambda rwkv, x, grad_cp=0, layout=None, carry=None: (
        seen.append(("blocks", grad_cp if torch.is_grad_enabled() else "nograd", carry is not None)), real_blocks(rwkv, x, grad_cp, layout, carry))[1])
    monkeypatch.setattr(fused, "head_loss", lambda head, x, plan: (seen.append(("head", plan.T)), real_head(head, x, plan))[1])
    ref = _visual(0, fused=False).float()
    cb = _batch("cpu")
    cb["images"] = {k: v.float() for k, v in cb["images"].items()}
    loss_ref, gref = _uncut(ref, cb)
    loss_gpu, g_gpu = _uncut(m, batch)
    seen.clear()
    for seg_len in (64, 32):
        K = T // seg_len
        for mode in (0, 1, 2):
            m.args.grad_cp = mode
            loss, grads = _cut(m, batch, seg_len)
            assert seen == [("blocks", "nograd", True)] * (K - 1) + [("blocks", mode, True), ("head", seg_len)] * K, seen
            seen.clear()
            worst = max(rel_rms(grads[n], g) for n, g in g_gpu.items() if g.abs().max() > 0 and g.numel() >= 64)
            print(f"[cut] seg_len {seg_len} grad_cp {mode}: loss {loss:.4f} (uncut GPU {loss_gpu:.4f}, fp32 CPU {loss_ref:.4f}); "
                  f"worst gradient group against the uncut GPU step: rel-RMS {worst:.2e}")
            assert abs(loss - loss_ref) < 1e-2 * abs(loss_ref), (seg_len, mode, loss, loss_ref)
            assert set(grads) == set(gref)
            checked = 0
            for n, gr in gref.items():
                if gr.abs().max() == 0 or gr.numel() < 64:
                    continue
                e = rel_rms(grads[n], gr)
                assert e < 2.6e-2, (seg_len, mode, n, e)
                if gr.numel() >= 1024:
                    group_bias(grads[n], gr, n, max_scale_err=8e-3)
                checked += 1
            assert checked >= 30


def test_cut_step_needs_less_memory_where_activations_dominate():
    """12 layers, C = 768, (2, 4096) cut into 4: the peak of the cut step is strictly below the uncut step's."""
    m = _visual(0, n_embd=768, dim_att=768, n_layer=12, ctx_len=4096).bfloat16().cuda()
    batch = _batch("cuda", 4096, image=False)
    peaks = {}
    for name, step in (("uncut", lambda: _uncut(m, batch)), ("cut", lambda: _cut(m, batch, 1024))):
        m.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        loss, _ = step()
        torch.cuda.synchronize()
        peaks[name] = (torch.cuda.max_memory_allocated(), base, loss)
    print(f"[cut] 12 x 768, (2, 4096): peak uncut {peaks['uncut'][0] / 2**20:.0f} MiB, cut in 4 {peaks['cut'][0] / 2**20:.0f} MiB "
          f"(allocated before the step: {peaks['uncut'][1] / 2**20:.0f} MiB); loss {peaks['uncut'][2]:.4f} / {peaks['cut'][2]:.4f}")
    assert peaks["cut"][0] < peaks["uncut"][0], peaks
