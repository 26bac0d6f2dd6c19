"""What the new pieces of the RWKV vision encoder (args.n_vrwkv_layer, VisualRWKV-v7/v7.10 `vrwkv`) cost on one MI355X at v7.10's geometry:
256 x 256 images, patch 16 (256 tokens per image), B_img images, n_embd = C.  One process; every leg runs under its own alarm.  Rounds alternate
the candidates; `iters` back-to-back calls per round are timed with HIP events; medians and the relative spread over the rounds are printed.

  --leg wgrad : vrwkv_patch_embed_wgrad_bf16 (dW and dbias straight from the pixels) against the composite in the same process: F.unfold (an
                unfolded copy of the images in HBM) + vrwkv_wgrad_big_bf16 + a column sum, and F.unfold + torch's matmul + sum.
  --leg tail  : through autograd, forward and forward + backward -- fused.ln_scatter_mean (+ head) against the composite behind VRWKV_TAIL=0:
                fused.add_ln, index_copy into the embedding rows, mean over tokens.
  --leg stack : forward + backward of a 6-Block VRWKV through fused.vrwkv_forward, with the kernels and with both composites.
Prints one JSON line per leg.
    python benchmarks/vrwkv_micro.py --leg wgrad|tail|stack [--B 16] [--C 2048] [--rounds 10] [--iters 10] [--out FILE]"""
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

PEAK_BF16_TFLOPS = 2517.0          # MI355X dense bf16 matrix-core peak (16 x the 157.3 TFLOPS fp32 matrix rate)


class _Alarm:
    """A time limit around one GPU leg: the process ends instead of going on after something hung."""

    def __init__(self, seconds, what):
        self.seconds, self.what = seconds, what

    def __enter__(self):
        def stop(*_):
            print(json.dumps({"bench": "vrwkv_micro", "leg": self.what, "error": f"time limit of {self.seconds} s"}), flush=True)
            os._exit(124)
        signal.signal(signal.SIGALRM, stop)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def alternate(a, fns):
    """{name: median ms, name_spread_rel: (max - min) / median over the rounds}."""
    def t(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters
    for _ in range(a.warmup):
        for fn in fns.values():
            t(fn)
    times = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            times[k].append(t(fn))
    res = {}
    for k, v in times.items():
        res[f"{k}_ms"] = round(statistics.median(v), 4)
        res[f"{k}_spread_rel"] = round((max(v) - min(v)) / statistics.median(v), 4)
    return res


def base(a, leg):
    return {"bench": "vrwkv_micro", "leg": leg, "B_img": a.B, "image": a.image, "patch": 16, "tokens_per_image": (a.image // 16) ** 2, "C": a.C,
            "rounds": a.rounds, "iters": a.iters, "device": torch.cuda.get_device_name(0)}


def leg_wgrad(a):
    from visualrwkv_amd import fused, hip_lib
    lib = hip_lib.load()
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(7)
    B, H, N = a.B, a.image, a.C
    M = B * (H // 16) ** 2
    px = (torch.randn(B, 3, H, H, device=dev, generator=g) * 0.5).bfloat16()
    do = (torch.randn(M, N, device=dev, generator=g) * 0.3).bfloat16()
    dw, db = torch.empty(N, 768, device=dev, dtype=torch.bfloat16), torch.empty(N, device=dev, dtype=torch.bfloat16)
    ws = torch.empty(lib.vrwkv_patch_embed_wgrad_ws_floats(B, H, H, 16, N), device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def kernel():
        assert lib.vrwkv_patch_embed_wgrad_bf16(B, H, H, 16, N, px.data_ptr(), do.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), st) == 0

    def unfold():
        return F.unfold(px, 16, stride=16).transpose(1, 2).reshape(M, 768)

    def comp_big():
        return fused.wgrad_big(do, unfold()), do.sum(0, dtype=torch.float32).bfloat16()

    def comp_torch():
        return do.t() @ unfold(), do.sum(0, dtype=torch.float32).bfloat16()

    kernel()
    ref_w, ref_b = comp_torch()
    res = base(a, "wgrad")
    res["rows"] = M
    res["max_abs_diff_vs_torch"] = round(float((dw.float() - ref_w.float()).abs().max()), 5)
    res["max_abs_diff_bias_vs_torch"] = round(float((db.float() - ref_b.float()).abs().max()), 5)
    fns = {"kernel": kernel, "unfold_torch": comp_torch}
    if fused.wgrad_big_supported(do, unfold()):
        fns["unfold_wgrad_big"] = comp_big
    res.update(alternate(a, fns))
    flops = 2.0 * M * N * 768
    res["kernel_matrix_core_fraction"] = round(flops / (res["kernel_ms"] * 1e-3) / (PEAK_BF16_TFLOPS * 1e12), 4)
    res["kernel_input_MB"] = round((px.numel() + do.numel()) * 2 / 1e6, 1)      # below the 256 MB Infinity Cache: repeated calls may be served from it
    res["kernel_input_TBps"] = round((px.numel() + 2 * do.numel()) * 2 / (res["kernel_ms"] * 1e-3) / 1e12, 3)     # dout is read by the GEMM and by the column sum
    for k in list(fns)[1:]:
        res[f"kernel_over_{k}"] = round(res["kernel_ms"] / res[f"{k}_ms"], 4)
    return res


def leg_tail(a):
    from visualrwkv_amd import fused
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(7)
    rnd = lambda *s, scale=1.0, shift=0.0: (torch.randn(*s, device=dev, generator=g) * scale + shift).bfloat16()
    B, L, C = a.B, (a.image // 16) ** 2, a.C
    rows_total = B * (L + 64)                    # every sample: its image tokens and 64 text tokens
    rows = torch.randperm(rows_total, device=dev, generator=g)[:B * L].sort().values.contiguous()
    x, delta = rnd(B, L, C).requires_grad_(True), rnd(B, L, C, scale=0.5).requires_grad_(True)
    embeds, gout, gp = rnd(rows_total, C), rnd(rows_total, C), rnd(B, C)
    ln = torch.nn.LayerNorm(C).to(dev).bfloat16()
    with torch.no_grad():
        ln.weight.copy_(rnd(C, scale=0.5, shift=1.0))
        ln.bias.copy_(rnd(C, scale=0.3))

    def fused_fwd():
        return fused.ln_scatter_mean(x, delta, ln, embeds.clone(), rows)

    def comp_fwd():
        _, h = fused.add_ln(x, delta, ln)
        return embeds.index_copy(0, rows, h.reshape(B * L, C)), h.mean(dim=1)

    def both(f):
        def run():
            x.grad = delta.grad = ln.weight.grad = ln.bias.grad = None
            out, pooled = f()
            torch.autograd.backward([out, pooled], [gout, gp])
        return run

    (a0, a1), (b0, b1) = fused_fwd(), comp_fwd()
    res = base(a, "tail")
    res["max_abs_diff_out"] = round(float((a0.detach().float() - b0.detach().float()).abs().max()), 5)
    res["max_abs_diff_pooled"] = round(float((a1.detach().float() - b1.detach().float()).abs().max()), 5)
    res["fwd"] = alternate(a, {"fused": fused_fwd, "composite": comp_fwd})
    res["fwd_bwd"] = alternate(a, {"fused": both(fused_fwd), "composite": both(comp_fwd)})
    nbytes = B * L * C * 2
    res["tensor_MB"] = round(nbytes / 1e6, 1)     # x, delta, xn, out: four such tensors plus the embedding clone -- compare with the 256 MB Infinity Cache
    for k in ("fwd", "fwd_bwd"):
        res[k]["fused_over_composite"] = round(res[k]["fused_ms"] / res[k]["composite_ms"], 4)
    return res


def leg_stack(a):
    from visualrwkv_amd import build, fused
    from visualrwkv_amd.rwkv7 import VRWKV
    build.build()
    dev = torch.device("cuda:0")
    B, C = a.B, a.C
    args = SimpleNamespace(n_embd=C, n_layer=24, n_vrwkv_layer=a.n_vrwkv_layer, dim_att=C, head_size_a=64, head_size_divisor=8, vocab_size=65536, dropout=0,
                           grad_cp=a.grad_cp, fused=True, image_size=a.image, patch_size=16)
    torch.manual_seed(42)
    ortho = torch.nn.init.orthogonal_
    torch.nn.init.orthogonal_ = lambda t, gain=1.0: t.normal_(0, 0.02 * gain)       # as bench.py --fast-init: the values do not matter here
    try:
        with torch.device(dev):
            m = VRWKV(args)
    finally:
        torch.nn.init.orthogonal_ = ortho
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() >= 2 and float(p.abs().max()) == 0.0:
                p.normal_(0, 0.01)
    m = m.to(torch.bfloat16)
    g = torch.Generator(device=dev).manual_seed(7)
    px = (torch.randn(B, 3, a.image, a.image, device=dev, generator=g) * 0.5).bfloat16()
    L = (a.image // 16) ** 2
    gf = (torch.randn(B, L, C, device=dev, generator=g) * 0.1).bfloat16()
    gl = (torch.randn(B, 1000, device=dev, generator=g) * 0.1).bfloat16()

    def run(wgrad, tail):
        def f():
            fused.PATCH_WGRAD, fused.VRWKV_TAIL = wgrad, tail
            m.zero_grad(set_to_none=True)
            feats, logits = fused.vrwkv_forward(m, px, grad_cp=a.grad_cp)
            torch.autograd.backward([feats, logits], [gf, gl])
        return f

    torch.cuda.reset_peak_memory_stats()
    res = base(a, "stack")
    res.update({"n_vrwkv_layer": a.n_vrwkv_layer, "grad_cp": a.grad_cp})
    try:
        res["fwd_bwd"] = alternate(a, {"kernels": run(True, True), "composite_wgrad": run(False, True), "composite_tail": run(True, False)})
    finally:
        fused.PATCH_WGRAD, fused.VRWKV_TAIL = True, True
    res["peak_GB"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["wgrad", "tail", "stack"], required=True)
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--image", type=int, default=256)
    ap.add_argument("--C", type=int, default=2048)
    ap.add_argument("--n-vrwkv-layer", type=int, default=6)
    ap.add_argument("--grad-cp", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=300, help="seconds the leg may take")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vrwkv_micro: needs an MI355X; a CPU run measures nothing")
    with _Alarm(a.limit, a.leg):
        out = {"wgrad": leg_wgrad, "tail": leg_tail, "stack": leg_stack}[a.leg](a)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
