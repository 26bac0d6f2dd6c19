"""Stateful RWKV-6 generation on the MI355X: the seven-launch decode step (decode6.py) against the module path on the same state, the
captured step against eager steps, one capture serving two prompts, and VisualRWKV6.generate_stateful against generate.

Two layers; C = 256 (LayerNorm outside the GEMV launches: the fold starts at 512; D = 32, d_decay = 64), C = 512 (the fold) and, for the
decode path alone, C = 4160 (65 heads: past the fold's 4096, where decode6.py goes back to the separate LayerNorm launch; D = 64,
d_decay = 128, the channel mix's value GEMV split over the waves); a prompt
of 24 tokens through the module path (RUN_CUDA_RWKV6_STATE takes any T), then 8 single tokens.  Bounds of the decode path against the
module path: those tests/test_stateful_gpu.py::test_decode_step_path_matches_module_path applies to RWKV-7, 2e-2 rel-RMS on logits, WKV
states and carried rows (two bf16 pipelines that round at different places)."""
from types import SimpleNamespace

import pytest
import torch

from oracle.wkv7_oracle import rel_rms
from tests.parity import NOTES

pytestmark = pytest.mark.gpu

PROMPT, STEPS = 24, 8
_MODELS = {}


def _lm(C):
    """One model per width for the module: bf16 on the GPU, every all-zero parameter (the LoRA first factors) given N(0, 0.05^2)."""
    if C not in _MODELS:
        from visualrwkv_amd.rwkv6 import RWKV
        torch.manual_seed(C)
        args = SimpleNamespace(n_embd=C, dim_att=C, n_layer=2, head_size_a=64, head_size_divisor=8, dim_ffn=C * 7 // 2, dropout=0, grad_cp=0,
                               vocab_size=320, fused=True)
        with torch.device("cuda" if C > 1024 else "cpu"):      # the wide model is drawn on the device: seconds of host time otherwise
            m = RWKV(args)
        with torch.no_grad():
            for p in m.parameters():
                if float(p.abs().sum()) == 0.0:
                    p.normal_(0, 0.05)
            for blk in m.blocks:
                for ln in (blk.ln1, blk.ln2):
                    ln.weight.normal_(1, 0.2); ln.bias.normal_(0, 0.1)
        _MODELS[C] = m.bfloat16().cuda().eval()
    return _MODELS[C]


def _tokens(B, C, seed=0):
    g = torch.Generator(device="cuda").manual_seed(1000 * B + C + seed)
    return (torch.randn(B, PROMPT + STEPS, C, device="cuda", generator=g) * 0.7).bfloat16()


def _state_tensors(st):
    return st.S + st.att_x + st.ffn_x


@pytest.mark.parametrize("C,B", [(256, 1), (256, 3), (512, 1), (512, 3), (4160, 2)])      # 4160: past the fold again, D = 64, d_decay = 128
def test_decode_step_path_matches_module_path(C, B):
    m = _lm(C)
    x = _tokens(B, C)
    _, st_a = m.forward_stateful(x[:, :PROMPT], None)
    _, st_b = m.forward_stateful(x[:, :PROMPT], None)
    for a, b in zip(_state_tensors(st_a), _state_tensors(st_b)):
        assert torch.equal(a, b)
    m.args.fused = False                                   # T = 1 forced eager: the module path
    try:
        ref = []
        for t in range(PROMPT, PROMPT + STEPS):
            lg, st_a = m.forward_stateful(x[:, t:t + 1], st_a, last_only=True)
            ref.append(lg)
    finally:
        m.args.fused = True
    for i, t in enumerate(range(PROMPT, PROMPT + STEPS)):
        lg, st_b = m.forward_stateful(x[:, t:t + 1], st_b, last_only=True)
        e = rel_rms(lg.float(), ref[i].float())
        if NOTES:
            print(f"[v6 stateful] C{C} B{B} step {i}: logits rel-RMS {e:.3e}")
        assert lg.shape == (B, 320) and e < 2e-2, (i, e)
    assert st_a.n_tokens == st_b.n_tokens == PROMPT + STEPS
    for a, b in zip(st_a.S, st_b.S):
        assert rel_rms(b, a) < 2e-2
    for a, b in zip(st_a.att_x + st_a.ffn_x, st_b.att_x + st_b.ffn_x):      # the carried token-shift rows
        assert rel_rms(b.float(), a.float()) < 2e-2


def test_decode_step_launch_count(monkeypatch):
    """Seven launches of the library per layer at C = 512, none of them a fallback to the module glue."""
    from visualrwkv_amd import hip_lib
    m = _lm(512)
    x = _tokens(1, 512)
    _, st = m.forward_stateful(x[:, :PROMPT], None)
    lib, calls = hip_lib.load(), []

    class Spy:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if not name.startswith("vrwkv_") or name == "vrwkv_strerror":
                return fn

            def wrapped(*a):
                calls.append(name)
                return fn(*a)
            return wrapped
    monkeypatch.setattr(hip_lib, "load", lambda: Spy())
    m.forward_stateful(x[:, PROMPT:PROMPT + 1], st, last_only=True)
    per_layer = ["vrwkv_gemv_ln_multi_bf16", "vrwkv_decode6_ddlerp_bf16", "vrwkv_gemv_multi_bf16", "vrwkv_decode6_tmix_head_bf16",
                 "vrwkv_gemv_multi_bf16", "vrwkv_gemv_ln_multi_bf16", "vrwkv_gemv_gated_copy_bf16"]
    assert calls == per_layer * 2 + ["vrwkv_gemv_multi_bf16"]              # + the head


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C", [256, 512])
def test_graph_decoder_equals_eager_steps(C, B):
    """The captured step replays the same kernels on the same state tensors: bit for bit over 8 tokens, logits and state."""
    m = _lm(C)
    x = _tokens(B, C, seed=1)
    _, st_a = m.forward_stateful(x[:, :PROMPT], None)
    _, st_b = m.forward_stateful(x[:, :PROMPT], None)
    dec = m.make_decoder(st_b)
    for a, b in zip(_state_tensors(st_a), _state_tensors(st_b)):            # warm-up and capture left the state as it was
        assert torch.equal(a, b)
    assert st_b.n_tokens == PROMPT
    for t in range(PROMPT, PROMPT + STEPS):
        want, st_a = m.forward_stateful(x[:, t:t + 1], st_a, last_only=True)
        got = dec(x[:, t:t + 1])
        assert torch.equal(got, want), t
    assert st_b.n_tokens == PROMPT + STEPS
    for a, b in zip(_state_tensors(st_a), _state_tensors(st_b)):
        assert torch.equal(a, b)


def test_decoder_for_reuses_one_capture_across_prompts():
    m = _lm(512)
    m.__dict__.pop("_decoders", None)
    decs = []
    for seed in (2, 3):
        x = _tokens(1, 512, seed=seed)
        _, st_a = m.forward_stateful(x[:, :PROMPT], None)
        _, st_b = m.forward_stateful(x[:, :PROMPT], None)
        dec = m.decoder_for(st_b)
        decs.append(dec)
        for t in range(PROMPT, PROMPT + 4):
            want, st_a = m.forward_stateful(x[:, t:t + 1], st_a, last_only=True)
            assert torch.equal(dec(x[:, t:t + 1]), want), (seed, t)
        for a, b in zip(_state_tensors(st_a), _state_tensors(dec.state)):
            assert torch.equal(a, b)
    assert decs[0] is decs[1] and len(m._decoders) == 1
    _, st3 = m.forward_stateful(_tokens(3, 512)[:, :PROMPT], None)          # another batch size: its own capture
    assert m.decoder_for(st3) is not decs[0]
    m.__dict__.pop("_decoders", None)


def test_generate_stateful_returns_generates_tokens():
    """image_state = 1 on the two-layer model of tests/test_v6_state_cpu.py (C = 128: no fold) with args.fused: the decode step, eager and
    from the captured graph, gives the tokens `generate` gives by re-running the text pass for every token."""
    from tests.test_v6_state_cpu import GOLD, _samples, _visual
    gold = torch.load(GOLD)
    m = _visual(gold, image_state=1).cuda().eval()
    m.args.fused = True
    s = _samples(gold)
    ids, images = s["input_ids"][:1].cuda(), s["images"][:1].cuda()
    want = m.generate(ids, images, False, 1.0, 1.0, 6, -1)
    assert len(want) == 6
    for use_graph in (False, True):
        assert m.generate_stateful(ids, images, False, 1.0, 1.0, 6, -1, use_graph=use_graph) == want, use_graph
    assert m.generate_stateful(ids, images, False, 1.0, 1.0, 6, want[2]) == want[:want.index(want[2]) + 1]
    m0 = _visual(gold, image_state=0).cuda().eval()                          # the model `generate` refuses
    m0.args.fused = True
    out = m0.generate_stateful(ids, images, False, 1.0, 1.0, 4, -1)
    assert len(out) == 4 and out == m0.generate_stateful(ids, images, False, 1.0, 1.0, 4, -1, use_graph=False)
