"""Cost of the carried state in the WKV6 kernels, alternated in one process:
  plain : vrwkv_wkv6_forward_bf16 / vrwkv_wkv6_backward_bf16
  state : vrwkv_wkv6_forward_state_bf16 (state0 in, state_T out) / vrwkv_wkv6_backward_state_bf16 (d_state_T in, d_state0 out)
at (B,T,H) = (2,2624,64) (cfg 4's operator) and (2,577,64) (the image pass of the v6.xx model).  Rounds alternate plain / state / plain / ...;
every round times `iters` back-to-back launches with HIP events after a warm-up.  One JSON line per shape and direction: median, min and
max of both, the spread of the plain rounds among themselves, and state / plain beside the derivable extra traffic (B x H x 16 KiB in and
out on top of the launch's own bytes).
--other-lib PATH: a second build of the library (e.g. the parent commit's); its PLAIN entries are alternated with this build's plain
entries in the same way ("other" in the output) -- the STATE = false instantiations should compile to the same code.
    python benchmarks/wkv6_state_micro.py [--rounds 12] [--iters 10] [--other-lib PATH] [--out profiles/wkv6_state_micro.jsonl]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from visualrwkv_amd import hip_lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--other-lib", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lib = hip_lib.load()
    other = None
    if a.other_lib:
        other = ctypes.CDLL(a.other_lib)
        for n in ("vrwkv_wkv6_forward_bf16", "vrwkv_wkv6_backward_bf16"):
            getattr(other, n).restype, getattr(other, n).argtypes = hip_lib.PROTOTYPES[n]
    dev = "cuda:0"
    st = torch.cuda.current_stream().cuda_stream
    P = lambda *ts: [t.data_ptr() for t in ts]
    lines = []

    def t(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters

    def alternate(f0, f1):
        for _ in range(a.warmup):
            t(f0); t(f1)
        t0, t1 = [], []
        for _ in range(a.rounds):
            t0.append(t(f0))
            t1.append(t(f1))
        return t0, t1

    for B, T, H in ((2, 2624, 64), (2, 577, 64)):
        C = H * 64
        g = torch.Generator(device=dev).manual_seed(T)
        uni = lambda *s, lo=-1.0, hi=1.0: (torch.rand(*s, device=dev, generator=g) * (hi - lo) + lo)
        r, k, v, gy = (uni(B, T, C).bfloat16() for _ in range(4))
        ew = (-torch.exp(uni(B, T, C, lo=-8.0, hi=1.0).bfloat16().float())).contiguous()
        u = uni(C).bfloat16()
        y = torch.empty_like(r)
        ck = torch.empty(lib.vrwkv_wkv6_ckpt_floats(B, T, H), dtype=torch.float32, device=dev)
        s0, dT = uni(B, H, 64, 64), uni(B, H, 64, 64)
        sT, d0 = torch.empty_like(s0), torch.empty_like(s0)
        outs = [torch.empty_like(r) for _ in range(4)] + [torch.empty(B, C, dtype=torch.bfloat16, device=dev)]
        elems = B * T * C
        launch_bytes = {"fwd": elems * (3 * 2 + 4 + 2) + ck.numel() * 4, "bwd": elems * (4 * 2 + 4 + 4 * 2) + ck.numel() * 4}
        extra_bytes = 2 * B * H * 64 * 64 * 4

        def fwd(l):
            return lambda: l.vrwkv_wkv6_forward_bf16(B, T, C, H, *P(r, k, v, ew, u, y, ck), st)

        def bwd(l):
            return lambda: l.vrwkv_wkv6_backward_bf16(B, T, C, H, *P(r, k, v, ew, u, gy, ck, *outs), st)

        fwd_state = lambda: lib.vrwkv_wkv6_forward_state_bf16(B, T, C, H, *P(r, k, v, ew, u, s0, y, sT, ck), st)
        bwd_state = lambda: lib.vrwkv_wkv6_backward_state_bf16(B, T, C, H, *P(r, k, v, ew, u, gy, ck, dT, *outs[:4], outs[4]), d0.data_ptr(), st)
        assert fwd_state() == 0 and bwd_state() == 0 and fwd(lib)() == 0 and bwd(lib)() == 0
        for kind, plain, state, mk in (("fwd", fwd(lib), fwd_state, fwd), ("bwd", bwd(lib), bwd_state, bwd)):
            tp, ts = alternate(plain, state)
            mp, ms = statistics.median(tp), statistics.median(ts)
            out = {"bench": "wkv6_state_micro", "kind": kind, "B": B, "T": T, "H": H, "rounds": a.rounds, "iters": a.iters,
                   "plain_ms_median": round(mp, 4), "plain_ms_min": round(min(tp), 4), "plain_ms_max": round(max(tp), 4),
                   "state_ms_median": round(ms, 4), "state_ms_min": round(min(ts), 4), "state_ms_max": round(max(ts), 4),
                   "plain_spread_rel": round((max(tp) - min(tp)) / mp, 4), "state_over_plain": round(ms / mp, 4),
                   "derived_extra_traffic_rel": round(extra_bytes / launch_bytes[kind], 4)}
            if other is not None:
                tq, to = alternate(plain, mk(other))
                mq, mo = statistics.median(tq), statistics.median(to)
                out.update({"vs_other_plain_ms_median": round(mq, 4), "other_plain_ms_median": round(mo, 4), "other_plain_ms_min": round(min(to), 4),
                            "other_plain_ms_max": round(max(to), 4), "vs_other_plain_spread_rel": round((max(tq) - min(tq)) / mq, 4),
                            "plain_over_other": round(mq / mo, 4)})
            out["device"] = torch.cuda.get_device_name(0)
            lines.append(json.dumps(out))
            print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
