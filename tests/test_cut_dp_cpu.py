"""VisualRWKV.train_step_cut under the ZeRO-1 engine on CPU: the step calls backward once per segment, so the engine's hooks fire several
times per parameter; inside Zero1Engine.hold_reductions() they only accumulate, and every bucket is reduced exactly once.  World size 2 over
gloo against the single-process cut step on the whole batch, compared as tests/test_dp_cpu.py::test_world4_gloo_with_a_rank_without_image
compares the engine on this model against a single process: the engine settings of its _ENG4 (eps = 1 makes the update nearly linear in the
gradient -- with 1e-8 a gradient that is zero up to rounding becomes a full +-lr step of either sign), replicas identical, and every
parameter's movement within 1e-3 of its largest movement + 1e-7."""
import os
import sys
from types import SimpleNamespace

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, V, STEPS, SEG = 32, 300, 3, 16


def _visual():
    from visualrwkv_amd.visual import VisualRWKV
    args = SimpleNamespace(n_embd=128, n_layer=2, dim_att=128, head_size_a=64, head_size_divisor=8, vocab_size=V, dropout=0, grad_cp=0, ctx_len=T,
                           num_token_per_image=16, vision_towers=("dino",), vision_image_size=56, load_model="", proj_type="mlp", weight_decay=0.0,
                           fused=False, vision_tower_kwargs={"dino": dict(depth=1, dim=64, heads=1)})
    torch.manual_seed(0)
    m = VisualRWKV(args)
    with torch.no_grad():
        for b in m.rwkv.blocks:
            b.att.output.weight.normal_(0, 0.05)
            b.ffn.value.weight.normal_(0, 0.05)
    m.freeze_proj()                              # text-only batches: the projector would never get a gradient
    return m.float()


def _batch(rows):
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, V, (2, T), generator=g)
    labels = ids.clone()
    labels[0, :5] = -100
    labels[1, 14:20] = -100
    return {"input_ids": ids[rows], "labels": labels[rows]}


def _train(m, batch):
    """STEPS cut steps under an engine with several buckets; returns (how far every parameter moved, reductions per bucket per step, losses)."""
    from visualrwkv_amd.dp import Zero1Engine
    eng = Zero1Engine(m, lr=0.5, betas=(0.9, 0.99), eps=1.0, weight_decay=0.0, grad_clip=1.0, bucket_mb=0.05)      # tests/test_dp_cpu.py::_ENG4
    init = [p.detach().clone() for p in m.parameters()]
    counts, losses = [], []
    real = eng._launch_reduce

    def counted(b):
        counts[-1][eng.buckets.index(b)] += 1
        return real(b)
    eng._launch_reduce = counted
    for _ in range(STEPS):
        counts.append([0] * len(eng.buckets))
        eng.zero_grad()
        losses.append(float(m.train_step_cut(batch, SEG)))
        eng.step()
    return [p.detach() - i for p, i in zip(m.parameters(), init)], counts, losses


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(4)
    params, counts, losses = _train(_visual(), _batch(slice(rank, 2, world)))
    torch.save({"params": params, "counts": counts, "losses": losses}, os.path.join(out_dir, f"r{rank}.pt"))
    dist.destroy_process_group()


def test_world2_cut_step_matches_single_process(tmp_path):
    port = 31500 + os.getpid() % 2000
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = torch.load(tmp_path / "r0.pt"), torch.load(tmp_path / "r1.pt")
    for a, b in zip(r0["params"], r1["params"]):
        assert torch.equal(a, b)                            # replicas stay identical
    for r in (r0, r1):                                      # exactly one reduction per bucket per step, on every rank
        assert len(r["counts"][0]) > 2 and all(c == [1] * len(c) for c in r["counts"]), r["counts"]
    params, counts, losses = _train(_visual(), _batch(slice(0, 2)))
    assert all(c == [1] * len(c) for c in counts), counts
    moved = 0
    for d_dp, d_one in zip(r0["params"], params):
        scale = float(d_one.abs().max())
        assert float((d_dp - d_one).abs().max()) <= 1e-3 * scale + 1e-7, (scale, float((d_dp - d_one).abs().max()))
        moved += int(scale > 0)
    assert moved > 40
    for i in range(STEPS):                                  # the batch mean of the two ranks' losses is the single process's loss
        assert abs(0.5 * (r0["losses"][i] + r1["losses"][i]) - losses[i]) < 1e-4 * abs(losses[i])


def test_hold_accumulates_over_backward_calls():
    """The engine alone: three backward calls inside hold_reductions() leave the sum of the three gradients, reduced once per bucket; the
    same three calls outside it are what the engine was never meant for (a bucket is launched as soon as its hooks have fired once)."""
    import torch.nn as nn
    from visualrwkv_amd.dp import Zero1Engine
    g = torch.Generator().manual_seed(1)
    xs, ys = torch.randn(3, 16, 24, generator=g), torch.randn(3, 16, 8, generator=g)
    for set_to_none in (True, False):
        torch.manual_seed(0)
        m = nn.Sequential(nn.Linear(24, 40), nn.LayerNorm(40), nn.Tanh(), nn.Linear(40, 8))
        ref = [torch.zeros_like(p) for p in m.parameters()]
        for x, y in zip(xs, ys):
            for r, gr in zip(ref, torch.autograd.grad(((m(x) - y) ** 2).mean(), list(m.parameters()))):
                r += gr
        eng = Zero1Engine(m, lr=1e-2, grad_clip=0.0, bucket_mb=0.001)
        launched = []
        real = eng._launch_reduce
        eng._launch_reduce = lambda b: (launched.append(eng.buckets.index(b)), real(b))[1]
        eng.zero_grad(set_to_none=set_to_none)
        with eng.hold_reductions():
            for x, y in zip(xs, ys):
                ((m(x) - y) ** 2).mean().backward()
            assert launched == []
        assert launched == list(range(len(eng.buckets))) and len(launched) > 1
        for p, r in zip(m.parameters(), ref):
            assert p.grad.data_ptr() >= eng.flat_grad.data_ptr()                  # .grad is (again) a view of the flat buffer
            assert torch.allclose(p.grad, r, rtol=1e-5, atol=1e-7)
        eng.step()
        eng.close()
