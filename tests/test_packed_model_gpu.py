"""Packed rows at the model level on the MI355X: training_step of a 2-layer C = 2048 VisualRWKV on a packed (2, 64) batch through the fused
path -- fused.blocks_forward with the layout (packed ln_mix shift kernels, packed WKV7 kernels) under its three memory modes, and the head on
the labelled rows with per-segment weights (fused.HeadPlan)."""
from types import SimpleNamespace

import pytest
import torch

from oracle.wkv7_oracle import rel_rms
from tests.parity import group_bias

pytestmark = pytest.mark.gpu

SEG_LENS = [[32, 32], [48, 16]]


def _visual(grad_cp, fused=True):
    """tests/test_wkv7_state_gpu.py::_visual without state_tune."""
    from visualrwkv_amd.visual import VisualRWKV
    args = SimpleNamespace(n_embd=2048, n_layer=2, dim_att=2048, head_size_a=64, head_size_divisor=8, vocab_size=65536,
                           dropout=0, grad_cp=grad_cp, ctx_len=64, num_token_per_image=16, vision_towers=("dino",),
                           vision_image_size=56, load_model="", proj_type="mlp", weight_decay=0.0, fused=fused,
                           check_image_tokens=not fused, vision_tower_kwargs={"dino": dict(depth=1, dim=64, heads=1)})
    torch.manual_seed(0)
    m = VisualRWKV(args)
    with torch.no_grad():
        for b in m.rwkv.blocks:
            b.att.output.weight.normal_(0, 0.02)
            b.ffn.value.weight.normal_(0, 0.02)
    m.freeze_emb()
    return m


def _batch(device):
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, 1000, (2, 64), generator=g)
    ids[0, 34:50] = 65535                                   # a 16-token image span inside segment 1 of row 0
    labels = ids.clone()
    labels[ids == 65535] = -100
    for r, row in enumerate(SEG_LENS):
        t = 0
        for n in row:
            labels[r, t:t + 4] = -100                       # first token of every segment (and a short prompt)
            t += n
    imgs = {"dino": torch.randn(1, 3, 56, 56, generator=g).bfloat16()}
    return {"input_ids": ids.to(device), "labels": labels.to(device), "sample_id": [["0", "1"], ["2", "3"]], "seg_lens": SEG_LENS, "n_samples": 4,
            "images": {k: v.to(device) for k, v in imgs.items()}}


def _step(m, batch):
    m.zero_grad(set_to_none=True)
    loss = m.training_step(batch)
    loss.backward()
    return float(loss.detach()), {n: p.grad.float().cpu() for n, p in m.named_parameters() if p.grad is not None}


def test_packed_step_under_every_memory_mode_and_against_fp32_cpu(monkeypatch):
    """The step takes fused.blocks_forward with the layout and fused.head_loss in every mode (counted).  grad_cp 0, 1, 2 agree to the bounds tests/test_wkv7_state_gpu.py holds the modes to (2e-3 on the loss, 4e-3 on gradients); the GPU
    step against an fp32 CPU evaluation of the same packed batch to the bounds of
    tests/test_model_gpu.py::test_full_visual_step_matches_an_independent_fp32_cpu_evaluation (1e-2 on the loss; every gradient group
    2.6e-2 rel-RMS, scale error of the larger groups 8e-3)."""
    from visualrwkv_amd import fused
    m = _visual(0).bfloat16().cuda()
    batch = _batch("cuda")
    seen = []
    real_blocks, real_head = fused.blocks_forward, fused.head_loss
    monkeypatch.setattr(fused, "blocks_forward", lambda rwkv, x, grad_cp=0, layout=None: (seen.append(("blocks", grad_cp, layout is not None)),
                                                                                          real_blocks(rwkv, x, grad_cp, layout))[1])
    monkeypatch.setattr(fused, "head_loss", lambda head, x, plan: (seen.append(("head",)), real_head(head, x, plan))[1])
    res = {}
    for mode in (0, 1, 2):
        m.args.grad_cp = mode
        res[mode] = _step(m, batch)
    assert seen == [("blocks", 0, True), ("head",), ("blocks", 1, True), ("head",), ("blocks", 2, True), ("head",)]
    for mode in (1, 2):
        assert abs(res[mode][0] - res[0][0]) < 2e-3 * abs(res[0][0]), (mode, res[mode][0], res[0][0])
        for n, gr in res[0][1].items():
            assert rel_rms(res[mode][1][n], gr) < 4e-3, (mode, n)
    ref = _visual(0, fused=False).float()
    cb = _batch("cpu")
    cb["images"] = {k: v.float() for k, v in cb["images"].items()}
    loss_ref, gref = _step(ref, cb)
    print(f"[packed] model step: GPU loss {res[0][0]:.4f}, fp32 CPU loss {loss_ref:.4f}")
    assert abs(res[0][0] - loss_ref) < 1e-2 * abs(loss_ref), (res[0][0], loss_ref)
    checked = 0
    for n, gr in gref.items():
        if gr.abs().max() == 0 or gr.numel() < 64:
            continue
        e = rel_rms(res[0][1][n], gr)
        assert e < 2.6e-2, (n, e)
        if gr.numel() >= 1024:
            group_bias(res[0][1][n], gr, n, max_scale_err=8e-3)
        checked += 1
    assert checked >= 30


def test_head_plan_with_a_layout_is_the_per_segment_loss():
    """fused.head_loss with HeadPlan(.., layout) against VisualRWKV.loss_from_logits(.., layout) on the same hidden state: the loss to the
    2e-3 the memory modes are held to above (bf16 loss against an fp32 one), and the hidden state's gradient to 4e-3."""
    import torch.nn.functional as F
    from visualrwkv_amd import fused
    from visualrwkv_amd.visual import VisualRWKV
    from visualrwkv_amd.wkv7 import PackedLayout
    g = torch.Generator().manual_seed(4)
    head = torch.nn.Linear(256, 4096, bias=False).bfloat16().cuda()
    h0 = torch.randn(2, 64, 256, generator=g).bfloat16().cuda()
    labels = _batch("cuda")["labels"].clamp(max=4095)
    lay = PackedLayout([[32, 16, 16], [48, 16]], 64, "cuda", n_samples=4)          # the last segment of row 0: a pad-only tail
    labels[0, 48:] = -100
    res = []
    for fn in (lambda h: fused.head_loss(head, h, fused.HeadPlan(labels, 0, -100, lay)),
               lambda h: VisualRWKV.loss_from_logits(F.linear(h, head.weight).float(), labels, lay)):
        h = h0.clone().requires_grad_(True)
        head.zero_grad(set_to_none=True)
        loss = fn(h)
        loss.backward()
        res.append((float(loss.detach()), h.grad.float().cpu(), head.weight.grad.float().cpu()))
    assert abs(res[0][0] - res[1][0]) < 2e-3 * abs(res[1][0]), (res[0][0], res[1][0])
    assert rel_rms(res[0][1], res[1][1]) < 4e-3 and rel_rms(res[0][2], res[1][2]) < 4e-3
    # rows that are the last of a segment carry no label
    plan = fused.HeadPlan(labels, 0, -100, lay)
    assert (plan.labels.view(2, 64)[0, [31, 47, 63]] == -100).all() and (plan.labels.view(2, 64)[1, [47, 63]] == -100).all()


def _hidden_and_input_grad(m, ids, lay, gout):
    x = m.rwkv.emb(ids).detach().requires_grad_(True)
    h, _ = m.rwkv(x, hidden_only=True, layout=lay)
    (h.float() * gout).sum().backward()
    return h.detach(), x.grad.detach()


def test_nothing_leaks_across_a_boundary():
    """Other token ids in segment 0 of row 0 only: the hidden rows of every other segment, and the gradient with respect to their input
    embedding rows, are the same BITS -- same shapes, same kernels, and those rows depend on nothing that changed."""
    from visualrwkv_amd.wkv7 import PackedLayout
    m = _visual(0).bfloat16().cuda()
    ids = _batch("cuda")["input_ids"].clamp(max=999)
    lay = PackedLayout(SEG_LENS, 64, "cuda")
    gout = torch.randn(2, 64, 2048, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    h0, g0 = _hidden_and_input_grad(m, ids, lay, gout)
    h1, g1 = _hidden_and_input_grad(m, ids, lay, gout)
    assert torch.equal(h0, h1) and torch.equal(g0, g1), "the step is not run-to-run deterministic at this shape"
    ids2 = ids.clone()
    ids2[0, :32] = (ids2[0, :32] + 7) % 1000
    h2, g2 = _hidden_and_input_grad(m, ids2, lay, gout)
    assert not torch.equal(h0[0, :32], h2[0, :32])
    assert torch.equal(h0[0, 32:], h2[0, 32:]) and torch.equal(h0[1], h2[1])
    assert torch.equal(g0[0, 32:], g2[0, 32:]) and torch.equal(g0[1], g2[1])


def test_nothing_leaks_through_the_packed_wkv7_op():
    """The package's own kernel alone, where no library GEMM is involved."""
    from oracle.wkv7_oracle import make_inputs
    from visualrwkv_amd import wkv7
    B, T, H = 2, 64, 32
    *ins, dy = [x.cuda() for x in make_inputs(B, T, H, seed=9)]
    lay = wkv7.PackedLayout(SEG_LENS, T, "cuda")

    def run(ins):
        leaves = [x.clone().requires_grad_(True) for x in ins]
        y = wkv7.WindBacksteppingPacked.apply(*leaves, lay)
        (y.float() * dy.float()).sum().backward()
        return y.detach(), [l.grad for l in leaves]
    y0, g0 = run(ins)
    other = [x.clone() for x in ins]
    for x, o in zip(other, make_inputs(B, T, H, seed=10)):
        x[0, :32] = o[0, :32].cuda()
    y1, g1 = run(other)
    assert not torch.equal(y0[0, :32], y1[0, :32])
    assert torch.equal(y0[0, 32:], y1[0, 32:]) and torch.equal(y0[1], y1[1])
    for a_, b_ in zip(g0, g1):
        assert torch.equal(a_[0, 32:], b_[0, 32:]) and torch.equal(a_[1], b_[1])
