"""State tuning (args.state_tune: a learnable initial WKV state per layer and head) on CPU tensors: the model layer on top of
RUN_CUDA_RWKV7g_state, whose CPU form is a plain PyTorch recurrence."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle.wkv7_oracle import rel_rms, wkv7_naive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lm_args(**kw):
    d = dict(n_embd=128, n_layer=2, dim_att=128, head_size_a=64, head_size_divisor=8, vocab_size=300, dropout=0,
             grad_cp=0, ctx_len=32, load_model="", num_token_per_image=16, proj_type="mlp")
    d.update(kw)
    return SimpleNamespace(**d)


def _lm(dtype=torch.float64, **kw):
    from visualrwkv_amd.rwkv7 import RWKV
    torch.manual_seed(3)
    m = RWKV(lm_args(**kw))
    with torch.no_grad():                        # zero-initialised projections would hide the state's effect
        for b in m.blocks:
            b.att.output.weight.normal_(0, 0.05)
            b.ffn.value.weight.normal_(0, 0.05)
    return m.to(dtype)


def _naive_plain(q, w, k, v, a, b):              # RUN_CUDA_RWKV7g's argument order
    B, T, HC = q.shape
    return wkv7_naive(*[i.view(B, T, HC // 64, 64) for i in (w, q, k, v, a, b)])[0].reshape(B, T, HC)


def _naive_state(q, w, k, v, a, b, state0, recompute_state=False):
    B, T, HC = q.shape
    s0 = state0.unsqueeze(0).expand(B, *state0.shape) if state0.dim() == 3 else state0
    y, fin = wkv7_naive(*[i.view(B, T, HC // 64, 64) for i in (w, q, k, v, a, b)], state0=s0)
    return y.reshape(B, T, HC), fin


def test_unset_switch_changes_nothing():
    """No parameter is created and the logits are the same tensor values whether the args object has no `state_tune` or has it 0."""
    a = _lm(torch.float32)
    b = _lm(torch.float32, state_tune=0)
    assert list(a.state_dict().keys()) == list(b.state_dict().keys())
    assert not any("time_state" in k for k in a.state_dict())
    x = torch.randn(2, 32, 128, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        assert torch.equal(a(x), b(x))


def test_zero_state_equals_the_stateless_model(monkeypatch):
    from visualrwkv_amd import rwkv7
    plain, tuned = _lm(), _lm(state_tune=1)
    extra = sorted(set(tuned.state_dict()) - set(plain.state_dict()))
    assert extra == ["blocks.0.att.time_state", "blocks.1.att.time_state"]
    assert tuple(tuned.blocks[0].att.time_state.shape) == (2, 64, 64) and float(tuned.blocks[0].att.time_state.detach().abs().max()) == 0.0
    tuned.load_state_dict(plain.state_dict(), strict=False)
    x = torch.randn(2, 32, 128, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    monkeypatch.setattr(rwkv7, "RUN_CUDA_RWKV7g", _naive_plain)          # the stateless op has no fp64 form
    with torch.no_grad():
        assert rel_rms(tuned(x), plain(x)) < 1e-12
    # fp32, every op the product's own (stateless: the host-core kernel behind the CPU key)
    monkeypatch.undo()
    p32, t32 = _lm(torch.float32), _lm(torch.float32, state_tune=1)
    with torch.no_grad():
        assert rel_rms(t32(x.float()), p32(x.float())) < 1e-5


def test_state_gradients_match_autograd_through_the_oracle(monkeypatch):
    from visualrwkv_amd import rwkv7
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 32, 128, dtype=torch.float64, generator=g)
    gout = torch.randn(2, 32, 300, dtype=torch.float64, generator=g)

    def run(patch):
        m = _lm(state_tune=1)
        with torch.no_grad():
            for b in m.blocks:
                b.att.time_state.normal_(0, 0.1, generator=torch.Generator().manual_seed(7 + b.layer_id))
        for n, p in m.named_parameters():
            p.requires_grad_(n.endswith(".time_state"))
        with monkeypatch.context() as mpc:
            if patch:
                mpc.setattr(rwkv7, "RUN_CUDA_RWKV7g_state", _naive_state)
            logits = m(x)
            (logits * gout).sum().backward()
        return logits.detach(), {n: p.grad for n, p in m.named_parameters()}

    lo, go = run(True)
    lp, gp = run(False)
    assert rel_rms(lp, lo) < 1e-12
    for n, gr in go.items():
        if n.endswith(".time_state"):
            assert gr is not None and float(gr.abs().max()) > 0 and rel_rms(gp[n], gr) < 1e-12, n
        else:
            assert gr is None and gp[n] is None, n


def _visual(seed=0, dtype=torch.float32):
    from visualrwkv_amd.visual import VisualRWKV
    args = SimpleNamespace(n_embd=128, n_layer=2, dim_att=128, head_size_a=64, head_size_divisor=8, vocab_size=65536,
                           dropout=0, grad_cp=0, ctx_len=32, num_token_per_image=16, vision_towers=("dino",),
                           vision_image_size=56, load_model="", proj_type="mlp", weight_decay=0.1, fused=False, state_tune=1,
                           vision_tower_kwargs={"dino": dict(depth=1, dim=64, heads=1)})
    torch.manual_seed(seed)
    m = VisualRWKV(args)
    with torch.no_grad():
        for p in m.rwkv.parameters():
            if p.dim() >= 2 and float(p.abs().max()) == 0.0 and p.dim() != 3:
                p.normal_(0, 0.02)
    return m.to(dtype)


def _batch(n=4, seed=1):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, 1000, (n, 32), generator=g)
    labels = ids.clone(); labels[:, :4] = -100
    return {"input_ids": ids, "labels": labels, "sample_id": [str(i) for i in range(n)]}


def test_freeze_groups_and_a_few_adamw_steps():
    m = _visual()
    m.freeze_for_state_tuning()
    trainable = [n for n, p in m.named_parameters() if p.requires_grad]
    assert trainable == ["rwkv.blocks.0.att.time_state", "rwkv.blocks.1.att.time_state"]
    groups = m.optimizer_groups()
    assert len(groups) == 1 and groups[0]["weight_decay"] == 0.0 and len(groups[0]["params"]) == 2
    opt = torch.optim.AdamW(groups, lr=3e-2)
    batch, losses = _batch(), []
    for _ in range(6):
        opt.zero_grad()
        loss = m.training_step(batch)
        loss.backward()
        for n, p in m.named_parameters():
            assert (p.grad is not None and float(p.grad.abs().max()) > 0) == n.endswith(".time_state"), n
        opt.step()
        losses.append(float(loss))
    assert losses[-1] < losses[0], losses


def test_freeze_needs_the_switch():
    m = _visual()
    for b in m.rwkv.blocks:
        del b.att.time_state
    with pytest.raises(ValueError):
        m.freeze_for_state_tuning()


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from visualrwkv_amd.dp import Zero1Engine
    m = _visual()
    m.freeze_for_state_tuning()
    b = _batch()
    shard = {"input_ids": b["input_ids"][rank::world], "labels": b["labels"][rank::world], "sample_id": b["sample_id"][rank::world]}
    eng = Zero1Engine(m, lr=1e-2, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.1, grad_clip=1.0, bucket_mb=0.001)
    for _ in range(2):
        eng.zero_grad(); m.training_step(shard).backward(); eng.step()
    torch.save([p.detach().clone() for n, p in m.named_parameters() if n.endswith(".time_state")], os.path.join(out_dir, f"r{rank}.pt"))
    dist.destroy_process_group()


def test_zero1_world2_gloo_matches_single_process(tmp_path):
    """ZeRO-1 over a state-tuning model (only time_state trainable): two ranks on halves of the batch = one process on all of it."""
    from visualrwkv_amd.dp import Zero1Engine
    port = 31500 + os.getpid() % 2000
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0 = torch.load(tmp_path / "r0.pt"); r1 = torch.load(tmp_path / "r1.pt")
    for a, b in zip(r0, r1):
        assert torch.equal(a, b)
    m = _visual()
    m.freeze_for_state_tuning()
    eng = Zero1Engine(m, lr=1e-2, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.1, grad_clip=1.0, bucket_mb=0.001)
    assert eng.wd_boundary == 0                                  # the states are not decayed
    batch = _batch()
    for _ in range(2):
        eng.zero_grad(); m.training_step(batch).backward(); eng.step()
    mine = [p for n, p in m.named_parameters() if n.endswith(".time_state")]
    assert float(mine[0].abs().max()) > 0
    for a, b in zip(r0, mine):
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-6)       # the tolerance of tests/test_dp_cpu.py's world-2 case
