"""Sampled generation on the MI355X: the pick kernel as the last launch of the captured decode step (GraphDecoder(sampled=True)) against
the same call without the graph, against greedy decoding at top_p = 0, and against a loop that feeds emb(token) by hand through the
unsampled decoder.  A tiny model (C = 256, 3 layers, vocabulary 1000), bf16, fused."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

N_NEW = 12


def _visual():
    from visualrwkv_amd.visual import VisualRWKV
    args = SimpleNamespace(n_embd=256, n_layer=3, dim_att=256, head_size_a=64, head_size_divisor=8, vocab_size=1000,
                           dropout=0, grad_cp=0, ctx_len=128, num_token_per_image=16, vision_towers=("dino",),
                           vision_image_size=56, load_model="", proj_type="mlp", fused=True,
                           vision_tower_kwargs={"dino": dict(depth=2, dim=64, heads=1)})
    torch.manual_seed(0)
    m = VisualRWKV(args)
    with torch.no_grad():
        for b in m.rwkv.blocks:
            b.att.output.weight.normal_(0, 0.05)
            b.ffn.value.weight.normal_(0, 0.05)
        m.rwkv.head.weight.mul_(4.0)
    return m.bfloat16().cuda().eval()


def _prompt(B):
    g = torch.Generator().manual_seed(10 + B)
    ids = torch.randint(0, 256, (B, 27), generator=g).cuda()
    images = {"dino": torch.randn(B, 3, 56, 56, generator=g).cuda().bfloat16()}
    return ids, images


def gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.fixture(scope="module")
def model():
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return _visual()


@pytest.fixture(autouse=True)
def _quiet():
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)         # the prompts carry no image placeholders (the vocabulary has no room for one)
        yield


@pytest.mark.parametrize("B", [1, 3])
def test_graph_equals_the_eager_path(model, B):
    """Token for token and logit for logit; the probabilities come from the same kernel on the same logits: bit-identical."""
    ids, images = _prompt(B)
    for tau, top_p in ((1.0, 0.9), (1.7, 1.0)):
        a = model.generate_stateful(ids, images, True, tau, top_p, N_NEW, -7, use_graph=True, generator=gen(B))
        b = model.generate_stateful(ids, images, True, tau, top_p, N_NEW, -7, use_graph=False, generator=gen(B))
        assert len(a[0]) == N_NEW and a == b
        if B > 1:
            assert all(len(t) == B for t in a[0]) and len({tuple(t[b] for t in a[0]) for b in range(B)}) > 1


def _prompt_seeded(seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, 256, (1, 27), generator=g).cuda()
    return ids, {"dino": torch.randn(1, 3, 56, 56, generator=g).cuda().bfloat16()}


def _top_two_gaps(model, ids, images, toks):
    """The gap between the two largest logits of every step of the greedy run `toks` (eager steps)."""
    samples = {"input_ids": ids, "images": images, "labels": ids}
    gaps = []
    with torch.no_grad():
        x, _ = model.preparing_embedding(samples)
        x = model.rwkv.pad_left(x, 5)
        logits, state = model.rwkv.forward_stateful(x, None, last_only=True)
        for t in toks:
            top = logits.float().topk(2, dim=-1).values[0]
            gaps.append(float(top[0]) - float(top[1]))
            logits, state = model.rwkv.forward_stateful(model.rwkv.emb(torch.tensor([[t]], device="cuda")), state, last_only=True)
    return gaps


def test_top_p_zero_is_greedy(model):
    """top_p = 0 keeps the maximum and its ties, so on a run whose two largest bf16 logits never tie it is the greedy run.  (A tie is
    no rarity among 1000 bf16 logits: the prompt is the first of eight seeds whose greedy run has none, asserted here.)"""
    for seed in range(8):
        ids, images = _prompt_seeded(seed)
        want = model.generate_stateful(ids, images, False, 1.0, 1.0, N_NEW, -7)
        if min(_top_two_gaps(model, ids, images, want[0])) > 0:
            break
    else:
        raise AssertionError("every candidate prompt has a tie between its two largest logits")
    for use_graph in (True, False):
        got = model.generate_stateful(ids, images, True, 1.3, 0.0, N_NEW, -7, use_graph=use_graph, generator=gen(2))
        assert got[0] == want[0] and got[1] == want[1], use_graph
        # greedy reports softmax in bf16, the pick in fp32
        assert got[2] == pytest.approx(want[2], rel=2 ** -7)


@pytest.mark.parametrize("B", [1, 3])
def test_the_graph_feeds_itself(model, B):
    """After each replay x_in is emb[token] bit for bit, and the tokens are those of a loop that feeds emb(token) by hand through the
    unsampled decoder and calls sampling.pick on its logits."""
    from visualrwkv_amd import sampling
    rwkv = model.rwkv
    tau, top_p = 1.2, 0.95
    u_all = torch.rand(N_NEW, B, generator=gen(20 + B)).cuda()
    x = torch.randn(B, 32, 256, generator=gen(3)).cuda().bfloat16()
    emb = rwkv.emb.weight
    runs = []
    for sampled in (True, False):
        logits, state = rwkv.forward_stateful(x, None, last_only=True)
        dec = rwkv.decoder_for(state, sampled=sampled)
        assert dec.sampled == sampled and rwkv.decoder_for(dec.state, sampled=sampled) is dec
        toks = []
        if sampled:
            dec.pick.set(tau, top_p)
            tk = sampling.pick(logits.contiguous(), tau, top_p, u_all[0], emb, dec.x_in)[0].cpu()
            for i in range(1, N_NEW):
                toks.append(tk.tolist())
                assert torch.equal(dec.x_in[:, 0].view(torch.int16), emb[tk.long().cuda()].view(torch.int16)), i
                tk = dec.sample(u_all[i])[0]
            toks.append(tk.tolist())
            assert torch.equal(dec.x_in[:, 0].view(torch.int16), emb[tk.long().cuda()].view(torch.int16))
        else:
            for i in range(N_NEW):
                tk = sampling.pick(logits.contiguous(), tau, top_p, u_all[i])[0]
                toks.append(tk.tolist())
                logits = dec(rwkv.emb(tk.long().view(B, 1)))
        runs.append(toks)
    assert runs[0] == runs[1]
    assert rwkv.decoder_for(state, sampled=True) is not rwkv.decoder_for(state, sampled=False)      # the cache keeps both


def test_one_more_launch_per_step(model, monkeypatch):
    """The library entries of a sampled step are the greedy step's plus exactly one vrwkv_sample_pick_bf16 at the end."""
    from visualrwkv_amd import hip_lib
    from visualrwkv_amd.rwkv7 import GraphDecoder
    rwkv = model.rwkv
    x = torch.randn(1, 32, 256, generator=gen(4)).cuda().bfloat16()
    _, state = rwkv.forward_stateful(x, None, last_only=True)
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
    rwkv.forward_stateful(x[:, :1], state, last_only=True)
    greedy = list(calls)
    assert greedy and "vrwkv_sample_pick_bf16" not in greedy
    for sampled, want in ((False, greedy * 3), (True, (greedy + ["vrwkv_sample_pick_bf16"]) * 3)):       # two warm-up steps and the capture
        calls.clear()
        GraphDecoder(rwkv, state, sampled=sampled)
        assert calls == want, sampled


def test_stop_token_ends_a_sampled_run(model):
    ids, images = _prompt(1)
    full = model.generate_stateful(ids, images, True, 1.0, 0.9, N_NEW, -7, generator=gen(5))
    stop = full[0][3]
    cut = model.generate_stateful(ids, images, True, 1.0, 0.9, N_NEW, stop, generator=gen(5))
    n = full[0].index(stop) + 1
    assert cut[0] == full[0][:n] and cut[1] == full[1][:n] and cut[2] == full[2][:n]


def test_generate_samples_too(model):
    """The re-running `generate` with do_sample: the pick kernel on each pass's last row; the same generator gives the same run."""
    ids, images = _prompt(1)
    a = model.generate(ids, images, True, 1.0, 0.9, 3, -7, generator=gen(6))
    b = model.generate(ids, images, True, 1.0, 0.9, 3, -7, generator=gen(6))
    assert len(a[0]) == 3 and all(0 <= t < 1000 for t in a[0]) and a == b
