"""Cost of the carried state in the WKV7 backward, alternated in one process at the bench shape (16, 2624, 32):
  plain : vrwkv_wkv7_backward_bf16
  state : vrwkv_wkv7_backward_state_bf16 with s0, ds_final and ds0 set
Rounds alternate plain / state / plain / state ...; every round times `iters` back-to-back launches with HIP events.  Prints one JSON
line: median and min of both, the spread of the plain rounds among themselves, and the state / plain ratio against the derivable
extra traffic (2 x B x H x 16 KiB read + written on top of the launch's own bytes).
    python benchmarks/wkv7_state_micro.py [--B 16] [--rounds 12] [--iters 10] [--out profiles/wkv7_state_micro.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from benchmarks.wkv7_micro import synth_inputs  # noqa: E402
from visualrwkv_amd import hip_lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--T", type=int, default=2624)
    ap.add_argument("--H", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lib = hip_lib.load()
    B, T, H, dev = a.B, a.T, a.H, "cuda:0"
    w, q, k, v, z, aa, dy = synth_inputs(B, T, H, dev)
    y = torch.empty_like(v)
    s = torch.empty(B, H, T // 16, 64, 64, dtype=torch.float32, device=dev)
    sa = torch.empty(B, T, H, 64, dtype=torch.float32, device=dev)
    s0 = torch.randn(B, H, 64, 64, device=dev) * 0.1
    dsT = torch.randn(B, H, 64, 64, device=dev) * 0.1
    ds0 = torch.empty_like(s0)
    fin = torch.empty_like(s0)
    g = [torch.empty_like(w) for _ in range(6)]
    st = torch.cuda.current_stream().cuda_stream
    P = lambda *ts: [t.data_ptr() for t in ts]
    assert lib.vrwkv_wkv7_forward_state_bf16(B, T, H, *P(w, q, k, v, z, aa, y, s0, fin, s, sa), st) == 0

    def plain():
        assert lib.vrwkv_wkv7_backward_bf16(B, T, H, *P(w, q, k, v, z, aa, dy, s, sa, *g), st) == 0

    def state():
        assert lib.vrwkv_wkv7_backward_state_bf16(B, T, H, *P(w, q, k, v, z, aa, dy, s, sa, s0, dsT, ds0, *g), st) == 0

    def t(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters

    for _ in range(a.warmup):
        t(plain); t(state)
    tp, tst = [], []
    for _ in range(a.rounds):
        tp.append(t(plain))
        tst.append(t(state))
    elems = B * T * H * 64
    launch_bytes = elems * (7 * 2 + 4 + 6 * 2) + s.numel() * 4            # 7 bf16 in, sa, 6 bf16 out, checkpoints
    extra = (3 * B * H * 64 * 64 * 4) / launch_bytes                       # s0 and ds_final read, ds0 written
    mp, ms = statistics.median(tp), statistics.median(tst)
    out = {"bench": "wkv7_state_micro", "B": B, "T": T, "H": H, "variant": lib.vrwkv_wkv7_last_variant(1), "rounds": a.rounds, "iters": a.iters,
           "plain_ms_median": round(mp, 4), "plain_ms_min": round(min(tp), 4), "plain_ms_max": round(max(tp), 4),
           "state_ms_median": round(ms, 4), "state_ms_min": round(min(tst), 4), "state_ms_max": round(max(tst), 4),
           "plain_spread_rel": round((max(tp) - min(tp)) / mp, 4), "state_over_plain": round(ms / mp, 4),
           "derived_extra_traffic_rel": round(extra, 4), "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
