"""Stateful RWKV-6 generation at the configuration-4 width (C = 4096, H = 64, dim_ffn = 14336): ms per generated token of the decode step
(decode6.py), eager and from the captured HIP graph, behind prompts of 64 and 512 tokens; the same as a multiple of the time to read the
layer weights once at 8 TB/s (what bounds a B <= 4 decode); and the per-token cost of today's `VisualRWKV6.generate` -- one text pass
over the whole prompt from the image states -- at the same two lengths.  All legs alternate inside one process, `rounds` times; the
figures are medians with their spread (min .. max over the rounds).

python benchmarks/decode6_micro.py [n_layer=32] [tokens_per_round=32] [rounds=7] [batch=1]        -> one JSON line"""
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from visualrwkv_amd.visual6 import VisualRWKV6  # noqa: E402

HBM_BYTES_PER_S = 8e12
PROMPTS = (64, 512)


def main():
    argv = [int(a) for a in sys.argv[1:]]
    n_layer, n_tok, rounds, B = (argv + [32, 32, 7, 1][len(argv):])[:4]
    C = 4096
    args = SimpleNamespace(n_embd=C, n_layer=n_layer, dim_att=C, dim_ffn=14336, head_size_a=64, head_size_divisor=8, vocab_size=65536,
                           dropout=0, grad_cp=0, ctx_len=4096, load_model="", fused=True, image_state=1, grid_size=-1)
    assert torch.cuda.is_available(), "decode6_micro measures on an MI355X"
    torch.manual_seed(0)
    with torch.device("cuda"):
        m = VisualRWKV6(args, nn.Identity(), 1024)          # generate's text pass needs no vision tower
        with torch.no_grad():
            for p in m.rwkv.parameters():
                if float(p.abs().sum()) == 0.0:
                    p.normal_(0, 0.02)
    m = m.bfloat16().eval()
    rwkv = m.rwkv
    layer_bytes = sum(p.numel() * p.element_size() for p in rwkv.blocks.parameters())
    step_bytes = layer_bytes + rwkv.head.weight.numel() * 2
    res = {"n_layer": n_layer, "batch": B, "tokens_per_round": n_tok, "rounds": rounds, "layer_weight_GB": round(layer_bytes / 1e9, 3),
           "weight_read_ms_at_8TBps": round(step_bytes / HBM_BYTES_PER_S * 1e3, 3)}
    g = torch.Generator(device="cuda").manual_seed(1)
    prompt = (torch.randn(B, max(PROMPTS), C, device="cuda", generator=g) * 0.5).bfloat16()
    x1 = (torch.randn(B, 1, C, device="cuda", generator=g) * 0.5).bfloat16()
    legs = {}
    with torch.no_grad():
        states = {}
        for L in PROMPTS:
            _, st_e = rwkv.forward_stateful(prompt[:, :L], None, last_only=True)
            _, st_g = rwkv.forward_stateful(prompt[:, :L], None, last_only=True)
            dec = rwkv.make_decoder(st_g)                    # one capture per leg: each replays on its own state tensors
            legs[f"eager_{L}"] = lambda st=st_e: rwkv.forward_stateful(x1, st, last_only=True)[0]
            legs[f"graph_{L}"] = lambda d=dec: d(x1)
            states[L] = [S.clone() for S in st_e.S]
            legs[f"generate_{L}"] = lambda L=L: m.text_forward(prompt[:1, :L], [S[:1] for S in states[L]])[:, -1]
        times = {k: [] for k in legs}
        for k, fn in legs.items():                           # warm up every shape the timed window uses
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for k, fn in legs.items():
                n = n_tok if not k.startswith("generate") else max(2, n_tok // 8)
                torch.cuda.synchronize(); t0 = time.perf_counter()
                for _ in range(n):
                    fn().argmax(-1).tolist()                 # the sampling step's host sync, as in generate / generate_stateful
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) / n * 1e3)
    for k, v in times.items():
        res[f"{k}_ms_per_token"] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
        if not k.startswith("generate"):
            res[f"{k}_x_weight_read"] = round(statistics.median(v) / (step_bytes / HBM_BYTES_PER_S * 1e3), 2)
    for mode in ("eager", "graph"):                          # the structural claim: a step costs the same behind 64 and 512 tokens
        a, b = times[f"{mode}_{PROMPTS[0]}"], times[f"{mode}_{PROMPTS[1]}"]
        res[f"{mode}_512_within_spread_of_64"] = bool(min(a) <= statistics.median(b) <= max(a) or min(b) <= statistics.median(a) <= max(b))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
