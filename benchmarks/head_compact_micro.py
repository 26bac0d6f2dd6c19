"""Backward of the head + loss node (fused._HeadCE) at the benchmark shape (16 x 2624 tokens, C 2048, V 65 536) for a range of labelled
fractions: the compact backward (dense on the labelled rows only) against the dense one (every row), ms per backward, HIP events, with the
shipped TunableOp file.  Where the two cross sets fused.HEAD_COMPACT_MAX_FRACTION.
    python benchmarks/head_compact_micro.py [out.jsonl]"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from visualrwkv_amd import fused  # noqa: E402
from visualrwkv_amd.gemm_tuning import enable_tuned_gemms  # noqa: E402


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
    enable_tuned_gemms()
    B, T, C, V = 16, 2624, 2048, 65536
    g = torch.Generator(device="cuda").manual_seed(0)
    head = torch.nn.Linear(C, V, bias=False, device="cuda", dtype=torch.bfloat16)
    with torch.no_grad():
        head.weight.copy_(torch.randn(V, C, device="cuda", generator=g) * 0.02)
    x0 = torch.randn(B, T, C, device="cuda", generator=g).bfloat16()
    limit = fused.HEAD_COMPACT_MAX_FRACTION
    for frac in (0.4, 0.6, 0.8, 0.85, 0.9, 0.95):
        labels = torch.randint(0, V, (B, T), device="cuda", generator=g)
        labels[:, : T - int(frac * T)] = -100                 # the prompt first, the answer labelled (the last row has no target)
        row = {"labelled_fraction": round(float((labels[:, 1:] >= 0).sum()) / (B * T), 4)}
        for mode, lim in (("dense", -1.0), ("compact", 2.0)):
            fused.HEAD_COMPACT_MAX_FRACTION = lim
            ts = []
            for _ in range(4):
                head.weight.grad = None
                x = x0.clone().requires_grad_(True)
                loss = fused.head_loss(head, x, fused.HeadPlan(labels, 0))
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                loss.backward()
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1))
            row[f"{mode}_ms"] = round(sorted(ts[1:])[1], 3)
        fused.HEAD_COMPACT_MAX_FRACTION = limit
        line = json.dumps(row)
        print(line)
        if out:
            out.write(line + "\n")


if __name__ == "__main__":
    main()
