"""What modality routing (args.modality_ffn: ln_v / ffn_v for image tokens, VisualRWKV-v7/v7.10) costs in the channel-mix token-shift kernels and
in a training step.  One process; every GPU leg runs under its own alarm.

  --leg kernels : at (B, T, C) = (16, 2624, 2048), rounds alternating  plain M = 1 / plain again (A/A) / routed with 576 image tokens per row
                  (one block after a 4-token prefix, bench.synthetic_batch's layout) / routed with 80 % image tokens (packed LLaVA rows: image
                  blocks of 576 with text between) / routed with the expert changing on every row (the worst case: the backward's register
                  set changes per row); forward and backward; `iters` back-to-back launches per round timed with HIP events.
  --leg step    : forward + backward of bench.py's 1.5 B configuration (no optimizer step, one synthetic batch with 576 image tokens per row)
                  for  the v7.00 model / modality_ffn routed / modality_ffn with BOTH channel mixes on every row through the same fused
                  kernels and a select (the reference's statement).
Prints one JSON line per leg.
    python benchmarks/routed_micro.py --leg kernels [--rounds 10] [--iters 10] [--out FILE]
    python benchmarks/routed_micro.py --leg step [--micro-bsz 16] [--steps 3] [--grad-cp 0] [--out FILE]"""
import argparse
import ctypes
import json
import os
import signal
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _Alarm:
    """A time limit around one GPU leg: the process ends instead of going on after something hung."""

    def __init__(self, seconds, what):
        self.seconds, self.what = seconds, what

    def __enter__(self):
        def stop(*_):
            print(json.dumps({"bench": "routed_micro", "leg": self.what, "error": f"time limit of {self.seconds} s"}), flush=True)
            os._exit(124)
        signal.signal(signal.SIGALRM, stop)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def masks(B, T):
    one = torch.zeros(B, T, dtype=torch.bool)
    one[:, 4:4 + 576] = True
    n = torch.arange(T)
    dense = ((n % 720) < 576).expand(B, T).clone()          # 576 image tokens, 144 of text, repeated: 80 %
    alt = (n % 2 == 1).expand(B, T).clone()
    return {"img576": one, "img80pct": dense, "alternating": alt}


def leg_kernels(a):
    from visualrwkv_amd import fused, hip_lib
    lib = hip_lib.load()
    B, T, C, dev = a.B, a.T, a.C, "cuda:0"
    ntok = B * T
    g = torch.Generator(device=dev).manual_seed(7)
    rnd = lambda *s, scale=1.0, shift=0.0: (torch.randn(*s, device=dev, generator=g) * scale + shift).bfloat16()
    x, delta, dout, dres = rnd(ntok, C), rnd(ntok, C, scale=0.5), rnd(ntok, C), rnd(ntok, C)
    w, b = [rnd(C, scale=0.5, shift=1.0) for _ in range(2)], [rnd(C, scale=0.3) for _ in range(2)]
    mu = [torch.rand(C, device=dev, generator=g).bfloat16() for _ in range(2)]
    xn, out, dx = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    mean, rstd = torch.empty(ntok, device=dev), torch.empty(ntok, device=dev)
    dwb, dmu = torch.empty(4, C, device=dev), torch.empty(2, C, device=dev)
    ws = torch.empty(max(lib.vrwkv_ln_mix_ws_floats(ntok, C, 1), lib.vrwkv_ln_mix_routed_ws_floats(ntok, C)), device=dev)
    st = torch.cuda.current_stream().cuda_stream
    arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    plans = {k: fused.RoutePlan(m.to(dev)) for k, m in masks(B, T).items()}

    def fwd_plain():
        assert lib.vrwkv_ln_mix_fwd_packed_bf16(ntok, T, C, 1e-5, 1, x.data_ptr(), delta.data_ptr(), w[0].data_ptr(), b[0].data_ptr(), arr([mu[0]]), xn.data_ptr(),
                                                arr([out]), mean.data_ptr(), rstd.data_ptr(), 0, st) == 0

    def bwd_plain():
        assert lib.vrwkv_ln_mix_bwd_packed_bf16(ntok, T, C, 1, xn.data_ptr(), mean.data_ptr(), rstd.data_ptr(), w[0].data_ptr(), b[0].data_ptr(), arr([mu[0]]),
                                                arr([dout]), 0, dres.data_ptr(), 0, dx.data_ptr(), dwb.data_ptr(), dmu.data_ptr(), ws.data_ptr(), st) == 0

    def fwd_routed(p):
        def f():
            assert lib.vrwkv_ln_mix_routed_fwd_bf16(ntok, T, C, 1e-5, x.data_ptr(), delta.data_ptr(), arr(w), arr(b), arr(mu), xn.data_ptr(), out.data_ptr(),
                                                    mean.data_ptr(), rstd.data_ptr(), 0, p.sel.data_ptr(), p.pos.data_ptr(), 4, st) == 0
        return f

    def bwd_routed(p):
        def f():
            assert lib.vrwkv_ln_mix_routed_bwd_bf16(ntok, T, C, xn.data_ptr(), mean.data_ptr(), rstd.data_ptr(), arr(w), arr(b), arr(mu), dout.data_ptr(),
                                                    dres.data_ptr(), 0, p.sel.data_ptr(), p.pos.data_ptr(), 4, dx.data_ptr(), dwb.data_ptr(), dmu.data_ptr(),
                                                    ws.data_ptr(), st) == 0
        return f

    def gather(p):
        return lambda: fused.row_gather(out, p.pos)

    def t(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters

    res = {"bench": "routed_micro", "leg": "kernels", "B": B, "T": T, "C": C, "rounds": a.rounds, "iters": a.iters, "device": torch.cuda.get_device_name(0),
           "image_fraction": {k: round(p.n_v / ntok, 4) for k, p in plans.items()}}
    fwd_plain()
    names = ["plain", "plain_again"] + list(plans)
    for leg, fns in (("fwd", [fwd_plain, fwd_plain] + [fwd_routed(p) for p in plans.values()]),
                     ("bwd", [bwd_plain, bwd_plain] + [bwd_routed(p) for p in plans.values()]),
                     ("unroute", [gather(p) for p in plans.values()])):
        for fn in fns * a.warmup:
            t(fn)
        times = [[] for _ in fns]
        for _ in range(a.rounds):
            for i, fn in enumerate(fns):
                times[i].append(t(fn))
        med = [statistics.median(v) for v in times]
        if leg == "unroute":
            res[leg] = {f"{k}_ms": round(m, 4) for k, m in zip(plans, med)}
            continue
        res[leg] = {f"{k}_ms": round(m, 4) for k, m in zip(names, med)}
        res[leg]["plain_round_spread_rel"] = round((max(times[0] + times[1]) - min(times[0] + times[1])) / med[0], 4)
        for k, m in zip(names[1:], med[1:]):
            res[leg][f"{k}_over_plain"] = round(m / med[0], 4)
    return res


def leg_step(a):
    import bench
    from visualrwkv_amd import build, fused
    from visualrwkv_amd.visual import VisualRWKV
    build.build()
    dev = torch.device("cuda:0")
    towers = ("dino", "siglip")
    batch = bench.synthetic_batch(a.micro_bsz, a.ctx_len, 576, towers, dev, seed=1234)
    batch["n_image_tokens"] = a.micro_bsz * 576             # counted where the batch is made: no synchronisation in the step

    def make(modality):
        args = bench.build_args("1b5", a.ctx_len, 576, towers, a.grad_cp, True, 16)
        args.modality_ffn = modality
        torch.manual_seed(42)
        ortho = torch.nn.init.orthogonal_
        torch.nn.init.orthogonal_ = lambda t, gain=1.0: t.normal_(0, 0.02 * gain)       # as bench.py --fast-init: the values do not matter here
        try:
            with torch.device(dev):
                model = VisualRWKV(args)
        finally:
            torch.nn.init.orthogonal_ = ortho
        with torch.no_grad():
            for n, p in model.rwkv.named_parameters():
                if p.dim() >= 2 and float(p.abs().max()) == 0.0:
                    p.normal_(0, 0.01)
        model = model.to(torch.bfloat16)
        model.freeze_emb()
        return model

    def run(model, what):
        times, loss = [], None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        for i in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.zero_grad(set_to_none=True)
            loss = model.training_step(batch)
            loss.backward()
            torch.cuda.synchronize()
            if i >= a.warmup:
                times.append(time.perf_counter() - t0)
        return {"what": what, "steps": len(times), "step_s_median": round(statistics.median(times), 4), "step_s_min_max": [round(min(times), 4), round(max(times), 4)],
                "loss": round(float(loss.detach()), 4), "peak_GB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 1)}

    def cmix_both(block, x, att_out, plan, first=None, selective=False):
        """The reference's statement on the fused kernels: both LayerNorm + shift kernels and both channel mixes on every row, then the select."""
        x2, (k_t,) = fused.add_ln_mix(x, att_out, block.ln2, (block.ffn.x_k,), False, first)
        _, (k_v,) = fused.add_ln_mix(x, att_out, block.ln_v, (block.ffn_v.x_k,), False, first)
        return x2, torch.where(plan.mask, fused.cmix_from_mixed(block.ffn_v, k_v, recompute_relusq=selective),
                               fused.cmix_from_mixed(block.ffn, k_t, recompute_relusq=selective))

    out = {"bench": "routed_micro", "leg": "step", "model": "1b5", "micro_bsz": a.micro_bsz, "ctx_len": a.ctx_len, "grad_cp": a.grad_cp,
           "image_tokens_per_row": 576, "device": torch.cuda.get_device_name(0),
           "note": "forward + backward, no optimizer step; fused path; peak_GB includes the model and its gradients"}
    model = make(0)
    out["v700"] = run(model, "v7.00 Block")
    del model
    model = make(1)
    out["routed"] = run(model, "modality_ffn, routed")
    real = fused.cmix_routed
    fused.cmix_routed = cmix_both
    try:
        out["both"] = run(model, "modality_ffn, both channel mixes on every row + select")
    finally:
        fused.cmix_routed = real
    out["routed_again"] = run(model, "modality_ffn, routed (again)")
    for k in ("routed", "both", "routed_again"):
        out[k]["over_v700"] = round(out[k]["step_s_median"] / out["v700"]["step_s_median"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["kernels", "step"], required=True)
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--T", type=int, default=2624)
    ap.add_argument("--C", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--micro-bsz", type=int, default=16)
    ap.add_argument("--ctx-len", type=int, default=2624)
    ap.add_argument("--grad-cp", type=int, default=0)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=420, help="seconds the leg may take")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    with _Alarm(a.limit, a.leg):
        out = leg_kernels(a) if a.leg == "kernels" else leg_step(a)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
