"""What the glue of the visual token compressor (args.n_vtc_layer, VisualRWKV-v7/v7.03-v7.04) costs on one MI355X at the 1.5 B geometry:
B = 16 samples of 729 projected image tokens, left-padded to T = 736, C = 2048, pooled to Lout = 64, n_vtc_layer = 2.  One process; every leg
runs under its own alarm.  Rounds alternate the candidates; `iters` back-to-back calls per round are timed with HIP events; medians are printed.

  --leg kernels : through the C ABI -- vrwkv_flip_add_bf16 with and without delta (and torch's x.flip(1) / (x + delta).flip(1) beside it);
                  vrwkv_ln_pool_scatter_fwd_bf16 and vrwkv_ln_pool_gather_bwd_bf16 (delta given, scattered through a row index).
  --leg tail    : through autograd, forward and forward + backward -- fused.ln_pool_scatter against the composite of what existed before it:
                  fused.add_ln, torch permute / F.adaptive_avg_pool1d / permute, index_copy into the embedding rows.  The embedding tensor holds
                  B (Lout + 64) rows, so the composite's out-of-place index_copy moves little beside the (B, T, C) passes.
  --leg stack   : forward + backward of the two Blocks through fused.vtc_forward (flip_add carrying the pending residual add, v_first flipped once)
                  against the same _block_segment walk with torch .flip(1) on x, the pending delta and v_first on both sides of the reversed Block;
                  both end in fused.add_ln(ln_out).
Prints one JSON line per leg.
    python benchmarks/vtc_micro.py --leg kernels|tail|stack [--rounds 10] [--iters 10] [--out FILE]"""
import argparse
import json
import os
import signal
import statistics
import sys
from types import SimpleNamespace

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _Alarm:
    """A time limit around one GPU leg: the process ends instead of going on after something hung."""

    def __init__(self, seconds, what):
        self.seconds, self.what = seconds, what

    def __enter__(self):
        def stop(*_):
            print(json.dumps({"bench": "vtc_micro", "leg": self.what, "error": f"time limit of {self.seconds} s"}), flush=True)
            os._exit(124)
        signal.signal(signal.SIGALRM, stop)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def timer(a):
    def t(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters
    return t


def alternate(a, fns):
    """{name: median ms} and the relative spread of the first candidate over the rounds."""
    t = timer(a)
    for _ in range(a.warmup):
        for fn in fns.values():
            t(fn)
    times = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            times[k].append(t(fn))
    res = {f"{k}_ms": round(statistics.median(v), 4) for k, v in times.items()}
    first = next(iter(times.values()))
    res["round_spread_rel"] = round((max(first) - min(first)) / statistics.median(first), 4)
    return res


def inputs(a, dev):
    g = torch.Generator(device=dev).manual_seed(7)
    rnd = lambda *s, scale=1.0, shift=0.0: (torch.randn(*s, device=dev, generator=g) * scale + shift).bfloat16()
    B, T, C, Lout = a.B, a.T, a.C, a.Lout
    rows_total = B * (Lout + 64)
    rows = torch.randperm(rows_total, device=dev, generator=g)[:B * Lout].sort().values.contiguous()
    return SimpleNamespace(x=rnd(B, T, C), delta=rnd(B, T, C, scale=0.5), w=rnd(C, scale=0.5, shift=1.0), b=rnd(C, scale=0.3), rows=rows,
                           embeds=rnd(rows_total, C), dout=rnd(rows_total, C), rnd=rnd)


def leg_kernels(a):
    from visualrwkv_amd import hip_lib
    lib = hip_lib.load()
    dev = "cuda:0"
    B, T, C, Lout, pad = a.B, a.T, a.C, a.Lout, a.pad
    v = inputs(a, dev)
    out, xn, dx = torch.empty_like(v.x), torch.empty_like(v.x), torch.empty_like(v.x)
    mean, rstd = torch.empty(B * T, device=dev), torch.empty(B * T, device=dev)
    dwb = torch.empty(2, C, device=dev)
    ws = torch.empty(lib.vrwkv_add_ln_ws_floats(B * T, C), device=dev)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()

    def flip():
        assert lib.vrwkv_flip_add_bf16(B, T, C, p(v.x), 0, p(out), st) == 0

    def flip_add():
        assert lib.vrwkv_flip_add_bf16(B, T, C, p(v.x), p(v.delta), p(out), st) == 0

    def tail_fwd():
        assert lib.vrwkv_ln_pool_scatter_fwd_bf16(B, T, pad, Lout, C, 1e-5, p(v.x), p(v.delta), p(v.w), p(v.b), p(v.rows), p(xn), p(v.embeds), p(mean), p(rstd), st) == 0

    def tail_bwd():
        assert lib.vrwkv_ln_pool_gather_bwd_bf16(B, T, pad, Lout, C, p(v.dout), p(v.rows), p(xn), p(mean), p(rstd), p(v.w), p(dx), p(dwb), p(ws), st) == 0

    tail_fwd()
    nbytes = B * T * C * 2
    res = {"bench": "vtc_micro", "leg": "kernels", "B": B, "T": T, "pad": pad, "Lout": Lout, "C": C, "rounds": a.rounds, "iters": a.iters,
           "device": torch.cuda.get_device_name(0), "tensor_MB": round(nbytes / 1e6, 1)}
    res["flip"] = alternate(a, {"flip": flip, "flip_add": flip_add, "torch_flip": lambda: v.x.flip(1), "torch_add_flip": lambda: (v.x + v.delta).flip(1)})
    res["tail"] = alternate(a, {"fwd": tail_fwd, "bwd": tail_bwd})
    # bytes the algorithm needs: flip 2 passes, flip_add 3; tail fwd reads x, delta and writes xn (the pad rows apart), bwd reads xn and writes dx
    res["flip"]["flip_TBps"] = round(2 * nbytes / res["flip"]["flip_ms"] / 1e9, 2)
    res["flip"]["flip_add_TBps"] = round(3 * nbytes / res["flip"]["flip_add_ms"] / 1e9, 2)
    res["tail"]["fwd_TBps"] = round(3 * nbytes / res["tail"]["fwd_ms"] / 1e9, 2)
    res["tail"]["bwd_TBps"] = round(2 * nbytes / res["tail"]["bwd_ms"] / 1e9, 2)
    return res


def leg_tail(a):
    from visualrwkv_amd import fused
    dev = "cuda:0"
    B, T, C, Lout, pad = a.B, a.T, a.C, a.Lout, a.pad
    v = inputs(a, dev)
    ln = torch.nn.LayerNorm(C).to(dev).bfloat16()
    with torch.no_grad():
        ln.weight.copy_(v.w)
        ln.bias.copy_(v.b)
    x, delta = v.x.requires_grad_(True), v.delta.requires_grad_(True)
    gout = v.dout

    def fused_fwd():
        return fused.ln_pool_scatter(x, delta, ln, pad, Lout, v.embeds.clone(), v.rows)

    def comp_fwd():
        _, h = fused.add_ln(x, delta, ln)
        pooled = F.adaptive_avg_pool1d(h[:, pad:].permute(0, 2, 1), Lout).permute(0, 2, 1).reshape(B * Lout, C)
        return v.embeds.index_copy(0, v.rows, pooled)

    def both(f):
        def run():
            x.grad = delta.grad = ln.weight.grad = ln.bias.grad = None
            f().backward(gout)
        return run

    a_, b_ = fused_fwd(), comp_fwd()
    diff = float((a_.detach().float() - b_.detach().float()).abs().max())
    res = {"bench": "vtc_micro", "leg": "tail", "B": B, "T": T, "pad": pad, "Lout": Lout, "C": C, "rounds": a.rounds, "iters": a.iters,
           "device": torch.cuda.get_device_name(0), "max_abs_diff_fused_vs_composite": round(diff, 5)}
    res["fwd"] = alternate(a, {"fused": fused_fwd, "composite": comp_fwd})
    res["fwd_bwd"] = alternate(a, {"fused": both(fused_fwd), "composite": both(comp_fwd)})
    for k in ("fwd", "fwd_bwd"):
        res[k]["fused_over_composite"] = round(res[k]["fused_ms"] / res[k]["composite_ms"], 4)
    return res


def leg_stack(a):
    from visualrwkv_amd import build, fused
    from visualrwkv_amd.rwkv7 import VisualTokenCompressor
    build.build()
    dev = torch.device("cuda:0")
    B, T, C = a.B, a.T, a.C
    args = SimpleNamespace(n_embd=C, n_layer=24, n_vtc_layer=a.n_vtc_layer, dim_att=C, head_size_a=64, head_size_divisor=8, vocab_size=65536, dropout=0,
                           grad_cp=a.grad_cp, fused=True)
    torch.manual_seed(42)
    ortho = torch.nn.init.orthogonal_
    torch.nn.init.orthogonal_ = lambda t, gain=1.0: t.normal_(0, 0.02 * gain)       # as bench.py --fast-init: the values do not matter here
    try:
        with torch.device(dev):
            vtc = VisualTokenCompressor(args)
    finally:
        torch.nn.init.orthogonal_ = ortho
    with torch.no_grad():
        for p in vtc.parameters():
            if p.dim() >= 2 and float(p.abs().max()) == 0.0:
                p.normal_(0, 0.01)
    vtc = vtc.to(torch.bfloat16)
    v = inputs(a, dev)
    x0 = v.x.requires_grad_(True)
    gout = v.rnd(B, T, C)

    def torch_flips(x):
        x = vtc.blocks[0].ln0(x)
        v_first, delta = torch.empty_like(x), None
        for i, block in enumerate(vtc.blocks):
            rev = i % 2 == 1
            if rev:
                x, v_first, delta = x.flip(1), v_first.flip(1), (delta.flip(1) if delta is not None else None)
            x, delta, v_first = fused._block_segment(block, x, delta, v_first, a.grad_cp == 2)
            if rev:
                x, v_first, delta = x.flip(1), v_first.flip(1), (delta.flip(1) if delta is not None else None)
        return x, delta

    def run(walk):
        def f():
            vtc.zero_grad(set_to_none=True)
            x0.grad = None
            x, delta = walk()
            _, h = fused.add_ln(x, delta, vtc.ln_out)
            h.backward(gout)
        return f

    fns = {"vtc_forward": run(lambda: fused.vtc_forward(vtc, x0, a.grad_cp)), "torch_flips": run(lambda: torch_flips(x0))}
    with torch.no_grad():
        xa, da = fused.vtc_forward(vtc, x0)
        xb, db = torch_flips(x0)
        diff = float(((xa.float() + (da.float() if da is not None else 0)) - (xb.float() + (db.float() if db is not None else 0))).abs().max())
    torch.cuda.reset_peak_memory_stats()
    res = {"bench": "vtc_micro", "leg": "stack", "B": B, "T": T, "C": C, "n_vtc_layer": a.n_vtc_layer, "grad_cp": a.grad_cp, "rounds": a.rounds,
           "iters": a.iters, "device": torch.cuda.get_device_name(0), "max_abs_diff_of_the_two_walks": round(diff, 5)}
    res["fwd_bwd"] = alternate(a, fns)
    res["fwd_bwd"]["vtc_forward_over_torch_flips"] = round(res["fwd_bwd"]["vtc_forward_ms"] / res["fwd_bwd"]["torch_flips_ms"], 4)
    res["peak_GB"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["kernels", "tail", "stack"], required=True)
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--T", type=int, default=736)
    ap.add_argument("--pad", type=int, default=7)
    ap.add_argument("--Lout", type=int, default=64)
    ap.add_argument("--C", type=int, default=2048)
    ap.add_argument("--n-vtc-layer", type=int, default=2)
    ap.add_argument("--grad-cp", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=300, help="seconds the leg may take")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vtc_micro: needs an MI355X; a CPU run measures nothing")
    with _Alarm(a.limit, a.leg):
        out = {"kernels": leg_kernels, "tail": leg_tail, "stack": leg_stack}[a.leg](a)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
