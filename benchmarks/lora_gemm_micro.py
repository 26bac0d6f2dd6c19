"""The LoRA products of RWKV_Tmix_x070 (src/model.py:176,181-184) as the library runs them: x (M x 2048) @ w1 (2048 x r), h (M x r) @ w2 (r x 2048)
and their input gradients dy @ w^T, against the time of reading / writing the wide operand once; then the two WRITE-WIDE ones -- h @ w2 and
dh @ w1^T -- on csrc/skinny_up.h beside the library's tuned kernel, per (rank, layout of w), with the box's own stream-copy and fill rates as the
floor.  python benchmarks/lora_gemm_micro.py [--out FILE]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timeit(fn, iters=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


NBUF = 4      # distinct inputs and outputs cycled through: 4 x 172 MB of output pass between two uses of a buffer, more than the 256 MB MALL holds


def timeit_cycled(fn, iters=40):
    """fn(i) with i cycling over the NBUF buffer sets; us per call."""
    for i in range(2 * NBUF):
        fn(i % NBUF)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i % NBUF)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    from visualrwkv_amd import fused, hip_lib
    from visualrwkv_amd.gemm_tuning import enable_tuned_gemms
    enable_tuned_gemms()
    M, C = 16 * 2624, 2048
    dev = "cuda"
    lines = []

    def emit(rec):
        line = json.dumps({k: round(v, 1) if isinstance(v, float) else v for k, v in rec.items()})
        print(line, flush=True)
        lines.append(line)

    x = torch.randn(M, C, device=dev, dtype=torch.bfloat16)
    for r in (64, 96, 256):
        w1 = torch.randn(C, r, device=dev, dtype=torch.bfloat16) * 0.02
        w2 = torch.randn(r, C, device=dev, dtype=torch.bfloat16) * 0.02
        h = torch.randn(M, r, device=dev, dtype=torch.bfloat16)
        emit({"M": M, "C": C, "r": r,
              "down_x@w1_us": timeit(lambda: x @ w1), "up_h@w2_us": timeit(lambda: h @ w2),
              "dgrad_up_dy@w2T_us": timeit(lambda: x @ w2.t()), "dgrad_down_dh@w1T_us": timeit(lambda: h @ w1.t()),
              "wide_once_us_at_5TBps": M * C * 2 / 5e6})
    del x

    # ---- the write-wide products: own kernel beside the library, NBUF buffer sets each
    lib = hip_lib.load()
    st = hip_lib.launch_stream(torch.device(dev))
    outs = [torch.empty(M, C, device=dev, dtype=torch.bfloat16) for _ in range(NBUF)]
    srcs = [torch.randn(M, C, device=dev, dtype=torch.bfloat16) for _ in range(NBUF)]
    wide_bytes = M * C * 2
    copy_us = timeit_cycled(lambda i: hip_lib.check(lib.vrwkv_stream_copy(srcs[i].data_ptr(), outs[i].data_ptr(), wide_bytes, st), "stream_copy"))
    fill_us = timeit_cycled(lambda i: hip_lib.check(lib.vrwkv_stream_probe(1, srcs[i].data_ptr(), srcs[i].data_ptr(), outs[i].data_ptr(),
                                                                           outs[i].data_ptr(), wide_bytes, st), "stream_probe"))
    del srcs
    emit({"floor": "this box", "stream_copy_us": copy_us, "stream_copy_GBps": 2 * wide_bytes / copy_us / 1e3,      # read + write
          "fill_us": fill_us, "fill_GBps": wide_bytes / fill_us / 1e3})
    for r in (64, 96, 256, 32, 128, 160):         # the 1.5B model's three ranks first, then the other ranks the kernel takes (0.1B, 0.4B)
        for cxr in (0, 1):
            hs = [torch.randn(M, r, device=dev, dtype=torch.bfloat16) for _ in range(NBUF)]
            ws = [torch.randn((C, r) if cxr else (r, C), device=dev, dtype=torch.bfloat16) * 0.1 for _ in range(NBUF)]

            def lib_fn(i):
                torch.matmul(hs[i], ws[i].t() if cxr else ws[i], out=outs[i])

            def own_fn(i):
                hip_lib.check(lib.vrwkv_skinny_up_bf16(M, r, C, hs[i].data_ptr(), ws[i].data_ptr(), cxr, outs[i].data_ptr(), st), "skinny_up")

            # alternate the two arms (A B A B): the clock and other tenants of the box move both
            t = {"lib": [], "own": []}
            for _ in range(3):
                t["lib"].append(timeit_cycled(lib_fn))
                t["own"].append(timeit_cycled(own_fn))
            own_fn(0)
            got = outs[0].float()
            lib_fn(0)
            ref = outs[0].float()
            lib_us, own_us = sorted(t["lib"])[1], sorted(t["own"])[1]
            emit({"product": "dh@w1T (w C x r)" if cxr else "h@w2 (w r x C)", "M": M, "C": C, "r": r, "w_is_CxR": cxr,
                  "lib_us": lib_us, "own_us": own_us, "lib_us_all": [round(v, 1) for v in t["lib"]], "own_us_all": [round(v, 1) for v in t["own"]],
                  "lib_write_GBps": wide_bytes / lib_us / 1e3, "own_write_GBps": wide_bytes / own_us / 1e3,
                  "own_faster_pct": (lib_us / own_us - 1.0) * 100.0, "own_over_fill": own_us / fill_us,
                  "ships_on_own_kernel": bool(lib_us / own_us > 1.10), "dispatch_has_it": (r, cxr) in fused.SKINNY_UP_CASES,
                  "max_abs_diff_vs_lib": float((got - ref).abs().max()), "elements_differing": float((got != ref).float().mean())})
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
