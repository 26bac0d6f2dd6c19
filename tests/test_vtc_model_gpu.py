"""args.n_vtc_layer at the model level on the MI355X: training_step of the 2-layer C = 2048 VisualRWKV of tests/test_routed_model_gpu.py with a
2-Block visual token compressor and the tiny DINO tower, through the fused path -- ln_v as one add_ln, fused.vtc_forward (the Blocks through
_block_segment, vrwkv_flip_add_bf16 around Block 1 and once for v_first) and the tail kernels (ln_out + unpad + pool over tokens + scatter into the
placeholder rows) -- under its three memory modes, against the eager modules (`.flip(1)`, nn.LayerNorm, F.adaptive_avg_pool1d, masked_scatter) in
fp32 on the CPU.

Images are 70 x 70: 25 tokens each (the tower takes any multiple of its 14-pixel patch), two images per sample = 50 tokens, neither a multiple of
16 (pad 14) nor of num_token_per_image = 4 (50 -> 8: windows of 7 that overlap).  Row 0 holds the placeholders of two images; row 1 those of two
(`full`) or of one (`short`: 12 placeholders for 16 features, so the last four features get row -1 and are dropped in both directions, where the
eager path truncates and warns).

Bounds by value from tests/test_routed_model_gpu.py: the modes agree to 2e-3 on the loss and 4e-3 on gradients; GPU against fp32 CPU 1e-2 on the
loss, 2.6e-2 rel-RMS on every gradient group, scale error of the larger groups 8e-3."""
import copy
import warnings
from types import SimpleNamespace

import pytest
import torch

from oracle.wkv7_oracle import rel_rms
from tests.parity import group_bias

pytestmark = pytest.mark.gpu

IMG, L_IMG, NTPI = 70, 25, 4


def _visual(grad_cp, fused=True):
    from visualrwkv_amd.visual import VisualRWKV
    args = SimpleNamespace(n_embd=2048, n_layer=2, n_vtc_layer=2, dim_att=2048, head_size_a=64, head_size_divisor=8, vocab_size=65536,
                           dropout=0, grad_cp=grad_cp, ctx_len=64, num_token_per_image=NTPI, vision_towers=("dino",),
                           vision_image_size=IMG, load_model="", proj_type="mlp", weight_decay=0.0, fused=fused,
                           check_image_tokens=not fused, vision_tower_kwargs={"dino": dict(depth=1, dim=64, heads=1)})
    torch.manual_seed(0)
    m = VisualRWKV(args)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for blocks in (m.rwkv.blocks, m.vtc.blocks):
            for b in blocks:
                b.att.output.weight.copy_(torch.randn(b.att.output.weight.shape, generator=g) * 0.02)
                b.ffn.value.weight.copy_(torch.randn(b.ffn.value.weight.shape, generator=g) * 0.02)
        m.vtc.ln_out.weight.copy_(1.0 + 0.2 * torch.randn(2048, generator=g))       # a wrong ln_out would otherwise look like none
        m.vtc.ln_out.bias.copy_(0.2 * torch.randn(2048, generator=g))
    m.freeze_emb()
    return m


@pytest.fixture(scope="module")
def models():
    """(the bf16 model on the GPU with args.fused, its fp32 twin on the CPU without): built once -- the orthogonal initialisation of the C = 2048
    matrices takes ten times as long as a step -- and never stepped, so every test sees the same weights."""
    cpu = _visual(0, fused=False).float()
    gpu = copy.deepcopy(cpu)
    for mod in gpu.modules():                    # every module holds the argument object it was built from (the compressor's Blocks a copy)
        if isinstance(getattr(mod, "args", None), SimpleNamespace):
            mod.args.fused, mod.args.check_image_tokens = True, False
    return gpu.bfloat16().cuda(), cpu


def _batch(device, holes):
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, 1000, (2, 64), generator=g)
    ids[0, 18:18 + holes[0]] = 65535
    ids[1, 0:holes[1]] = 65535
    labels = ids.clone()
    labels[ids == 65535] = -100
    labels[:, :4] = -100
    imgs = {"dino": torch.randn(4, 3, IMG, IMG, generator=g).bfloat16()}
    return {"input_ids": ids.to(device), "labels": labels.to(device), "sample_id": ["0", "1"], "images": {k: v.to(device) for k, v in imgs.items()}}


def _step(m, batch):
    m.zero_grad(set_to_none=True)
    loss = m.training_step(batch)
    loss.backward()
    return float(loss.detach()), {n: p.grad.float().cpu() for n, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("case,holes", [("full", (8, 8)), ("short", (8, 4))])
def test_vtc_step_under_every_memory_mode_and_against_fp32_cpu(monkeypatch, models, case, holes):
    from visualrwkv_amd import fused
    m, ref = models
    assert m.args.fused and m.vtc.blocks[1].att.args.fused and not ref.args.fused
    batch = _batch("cuda", holes)
    seen, tails, flips = [], [], []
    real_fwd, real_tail, real_flip = fused.vtc_forward, fused.ln_pool_scatter, fused.flip_add
    monkeypatch.setattr(fused, "vtc_forward", lambda vtc, x, grad_cp=0, layout=None: (seen.append((grad_cp, tuple(x.shape))), real_fwd(vtc, x, grad_cp, layout))[1])
    monkeypatch.setattr(fused, "ln_pool_scatter", lambda x, delta, ln, pad, Lout, e=None, r=None: (
        tails.append((pad, Lout, delta is None, int((r < 0).sum()))), real_tail(x, delta, ln, pad, Lout, e, r))[1])
    monkeypatch.setattr(fused, "flip_add", lambda x, delta=None: (flips.append(delta is not None), real_flip(x, delta))[1])
    res = {}
    for mode in (0, 1, 2):
        m.args.grad_cp = mode
        flips.clear()
        res[mode] = _step(m, batch)
        # into Block 1 with Block 0's pending add, v_first once, out of Block 1 with its pending add (mode 1 re-runs the Blocks in the backward;
        # the flips stay outside the checkpoint)
        assert flips == [True, False, True], (mode, flips)
    assert seen == [(0, (2, 64, 2048)), (1, (2, 64, 2048)), (2, (2, 64, 2048))]
    n_drop = 16 - sum(holes)
    assert tails == [(14, 8, True, n_drop)] * 3, tails
    for mode in (1, 2):
        assert abs(res[mode][0] - res[0][0]) < 2e-3 * abs(res[0][0]), (mode, res[mode][0], res[0][0])
        for n, gr in res[0][1].items():
            assert rel_rms(res[mode][1][n], gr) < 4e-3, (mode, n)
    m.args.grad_cp = 0
    cb = _batch("cpu", holes)
    cb["images"] = {k: v.float() for k, v in cb["images"].items()}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # `short`: the eager path warns that it truncates
        loss_ref, gref = _step(ref, cb)
    print(f"[vtc] model step ({case}): GPU loss {res[0][0]:.4f}, fp32 CPU loss {loss_ref:.4f}")
    assert abs(res[0][0] - loss_ref) < 1e-2 * abs(loss_ref), (res[0][0], loss_ref)
    checked, vtc_groups = 0, 0
    assert set(gref) == set(res[0][1])
    for n, gr in gref.items():
        if gr.abs().max() == 0 or gr.numel() < 64:
            continue
        e = rel_rms(res[0][1][n], gr)
        print(f"[vtc] {n}: rel-RMS {e:.3e}")
        assert e < 2.6e-2, (n, e)
        if gr.numel() >= 1024:
            group_bias(res[0][1][n], gr, n, max_scale_err=8e-3)
        checked += 1
        vtc_groups += n.startswith("vtc.")
    assert checked >= 60 and vtc_groups >= 30, (checked, vtc_groups)


def test_compress_visual_tokens_on_the_gpu_is_the_eager_result(models):
    """The public method on the fused path (dense tail, and 'step' through add_ln + a slice) against the eager module on the same bf16 weights."""
    m = models[0]
    feats = (torch.randn(2, 2, L_IMG, 2048, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2)) * 0.5).bfloat16()
    with torch.no_grad():
        for red, n in (("pool", 8), ("step", 9)):
            got = m.compress_visual_tokens(feats, red)
            m.vtc.args.fused = False                 # the module's eager statement: .flip(1), nn.LayerNorm, F.adaptive_avg_pool1d
            try:
                want = m.compress_visual_tokens(feats, red)
            finally:
                m.vtc.args.fused = True
            assert got.shape == want.shape == (2, n, 2048)
            assert rel_rms(got.float().cpu(), want.float().cpu()) < 1e-2, red
