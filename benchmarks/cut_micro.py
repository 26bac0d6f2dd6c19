"""What training a row in segments costs and saves.  One process.  The alarm around a leg is a Python signal handler: it ends a leg that is
slow, not one that is stuck inside a HIP call (the handler runs between bytecodes), so run every leg under an external `timeout -k 10 <s>` too.

  --leg kernels : the token-shift entries at (B, T, C) = (16, 2624, 2048), rounds alternating  plain / plain (A/A) / the _carry entry with
                  every carry pointer NULL / the _carry entry with carries at both ends; forward M = 1 and 6, backward M = 1 and M = 6
                  (vrwkv_mix_bwd_ln_*); `iters` back-to-back launches per round timed with HIP events.  A _carry launch slower than plain
                  by more than the plain A/A spread is a finding.
  --leg step    : bench.py's 1.5 B configuration (built here from bench.build_args; no optimizer step) on one synthetic batch:
                  training_step + backward against train_step_cut with K = 2 and 4 segments -- step time and peak memory.
                  --micro-bsz 16 --ctx-len 2624 is the bench configuration, --micro-bsz 8 --ctx-len 6400 BASELINE's config 5.
Prints one JSON line per leg.
    python benchmarks/cut_micro.py --leg kernels [--rounds 10] [--iters 10] [--out FILE]
    python benchmarks/cut_micro.py --leg step [--micro-bsz 16] [--ctx-len 2624] [--steps 3] [--grad-cp 0] [--out FILE]"""
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
    """A time limit around one GPU leg: the process ends instead of going on when a leg takes too long.  It cannot interrupt a call that
    never returns (see the module docstring)."""

    def __init__(self, seconds, what):
        self.seconds, self.what = seconds, what

    def __enter__(self):
        def stop(*_):
            print(json.dumps({"bench": "cut_micro", "leg": self.what, "error": f"time limit of {self.seconds} s"}), flush=True)
            os._exit(124)
        signal.signal(signal.SIGALRM, stop)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def leg_kernels(a):
    from visualrwkv_amd import hip_lib
    lib = hip_lib.load()
    B, T, C, dev = a.B, a.T, a.C, "cuda:0"
    n = B * T
    g = torch.Generator(device=dev).manual_seed(1)
    mk = lambda *s: torch.randn(*s, generator=g, device=dev)
    x, d = mk(n, C).bfloat16(), (0.5 * mk(n, C)).bfloat16()
    w, b = (1 + 0.2 * mk(C)).bfloat16(), (0.1 * mk(C)).bfloat16()
    mus = [torch.rand(C, generator=g, device=dev).bfloat16() for _ in range(6)]
    douts = [mk(n, C).bfloat16() for _ in range(7)]
    y0, yl, dyT, dyp = mk(B, C).bfloat16(), torch.empty(B, C, dtype=torch.bfloat16, device=dev), mk(B, C), torch.empty(B, C, device=dev)
    xn, outs = torch.empty_like(x), [torch.empty_like(x) for _ in range(6)]
    mean, rstd = torch.empty(n, device=dev), torch.empty(n, device=dev)
    dx, dy, dmu, dwb = torch.empty_like(x), torch.empty_like(x), torch.empty(6, C, device=dev), torch.empty(2, C, device=dev)
    ws1 = torch.empty(lib.vrwkv_ln_mix_ws_floats(n, C, 1), device=dev)
    ws6 = torch.empty(max(1, lib.vrwkv_param_grad_ws_floats(n, C, 6)), device=dev)
    st = torch.cuda.current_stream().cuda_stream
    PA = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    p = lambda t: t.data_ptr() if t is not None else None

    def fwd(M, carry):
        head = (n, T, C, 1e-5, M, p(x), p(d), p(w), p(b), PA(mus[:M]), p(xn), PA(outs[:M]), p(mean), p(rstd))
        if carry is None:
            return lambda: lib.vrwkv_ln_mix_fwd_bf16(*head, st)
        return lambda: lib.vrwkv_ln_mix_fwd_carry_bf16(*head, *carry, st)

    def bwd1(carry):
        head = (n, T, C, 1, p(xn), p(mean), p(rstd), p(w), p(b), PA(mus[:1]), PA(douts[:1]), None, p(douts[6]))
        tail = (p(dx), p(dwb), p(dmu), p(ws1), st)
        if carry is None:
            return lambda: lib.vrwkv_ln_mix_bwd_bf16(*head, *tail)
        return lambda: lib.vrwkv_ln_mix_bwd_carry_bf16(*head, *carry, *tail)

    def bwd6(carry):
        head = (n, T, C, 6, p(xn), p(mean), p(rstd), p(w), p(b), PA(mus), PA(douts[:6]), p(douts[6]))
        tail = (p(dy), p(dmu), p(ws6), st)
        if carry is None:
            return lambda: lib.vrwkv_mix_bwd_ln_bf16(*head, *tail)
        return lambda: lib.vrwkv_mix_bwd_ln_carry_bf16(*head, *carry, *tail)

    def t(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            assert fn() == 0
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters

    out = {"bench": "cut_micro", "leg": "kernels", "B": B, "T": T, "C": C, "rounds": a.rounds, "iters": a.iters, "device": torch.cuda.get_device_name(0)}
    fc, fn0 = (p(y0), p(yl)), (None, None)
    bc, bn0 = (p(y0), p(dyT), p(dyp)), (None, None, None)
    assert fwd(1, None)() == 0                               # xn and the statistics the backward legs read
    for name, legs in (("fwd_M1", [fwd(1, None), fwd(1, None), fwd(1, fn0), fwd(1, fc)]), ("fwd_M6", [fwd(6, None), fwd(6, None), fwd(6, fn0), fwd(6, fc)]),
                       ("bwd_M1", [bwd1(None), bwd1(None), bwd1(bn0), bwd1(bc)]), ("bwd_M6", [bwd6(None), bwd6(None), bwd6(bn0), bwd6(bc)])):
        for fn in legs * a.warmup:
            t(fn)
        times = [[] for _ in legs]
        for _ in range(a.rounds):
            for i, fn in enumerate(legs):
                times[i].append(t(fn))
        med = [statistics.median(v) for v in times]
        out[name] = {"plain_ms": round(med[0], 4), "plain_again_ms": round(med[1], 4), "carry_null_ms": round(med[2], 4), "carry_ms": round(med[3], 4),
                     "plain_AA_rel": round(abs(med[1] - med[0]) / med[0], 4),
                     "plain_round_spread_rel": round((max(times[0] + times[1]) - min(times[0] + times[1])) / med[0], 4),
                     "null_over_plain": round(med[2] / med[0], 4), "carry_over_plain": round(med[3] / med[0], 4)}
    return out


def leg_step(a):
    import bench
    from visualrwkv_amd import build
    from visualrwkv_amd.visual import VisualRWKV
    build.build()
    dev = torch.device("cuda:0")
    towers = ("dino", "siglip")
    args = bench.build_args("1b5", a.ctx_len, 576, towers, a.grad_cp, True, 16)
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
    batch = bench.synthetic_batch(a.micro_bsz, a.ctx_len, 576, towers, dev, seed=1234)
    T = a.ctx_len

    def seg_len(K):                                          # K segments of whole chunks, the last one the shortest
        return -(-T // (16 * K)) * 16

    def uncut():
        loss = model.training_step(batch)
        loss.backward()
        return loss.detach()

    def run(step, what):
        times, loss = [], None
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        for i in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.zero_grad(set_to_none=True)
            loss = step()
            torch.cuda.synchronize()
            if i >= a.warmup:
                times.append(time.perf_counter() - t0)
        return {"what": what, "steps": len(times), "step_s_median": round(statistics.median(times), 4), "step_s_min_max": [round(min(times), 4), round(max(times), 4)],
                "loss": round(float(loss), 4), "peak_GB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 1)}

    out = {"bench": "cut_micro", "leg": "step", "model": "1b5", "micro_bsz": a.micro_bsz, "ctx_len": T, "grad_cp": a.grad_cp,
           "device": torch.cuda.get_device_name(0), "note": "forward + backward, no optimizer step; fused path; peak_GB includes the model and its gradients"}
    legs = [("uncut", uncut)] if not a.skip_uncut else []
    for K in a.K:
        legs.append((f"cut_K{K}", lambda K=K: model.train_step_cut(batch, seg_len(K))))
    if not a.skip_uncut:
        legs.append(("uncut_again", uncut))
    for name, step in legs:
        out[name] = run(step, name)
        if name.startswith("cut_K"):
            out[name]["seg_len"] = seg_len(int(name[5:]))
            if "uncut" in out:
                out[name]["time_over_uncut"] = round(out[name]["step_s_median"] / out["uncut"]["step_s_median"], 3)
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
    ap.add_argument("--K", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--skip-uncut", action="store_true", help="the uncut step does not fit (a long row at a large micro-batch): cut legs only")
    ap.add_argument("--limit", type=int, default=420, help="seconds the leg may take")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    with _Alarm(a.limit, a.leg):
        out = leg_kernels(a) if a.leg == "kernels" else leg_step(a)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
