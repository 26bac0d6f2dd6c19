"""What sample packing costs in the WKV7 kernels and what it buys in a training step.  One process; every GPU leg runs under its own alarm.

  --leg kernels : at (B, T, H) = (16, 2624, 32), rounds alternating  plain / plain (A/A) / packed with all-zero flags / packed with a seeded
                  layout of several samples per row (segment lengths 16 * U{1..60}), forward and backward; `iters` back-to-back launches per
                  round timed with HIP events.  A packed launch slower than plain by more than the plain A/A spread is a finding.
  --leg step    : forward + backward of bench.py's 1.5 B configuration (built here from bench.build_args; no optimizer step) on the SAME stream
                  of samples, once through the padded collate (every sample right-padded to ctx_len) and once through data.pack_batches.  Sample
                  lengths: the ten records of tests/golden/data_ref.pt tokenised with its recorded token table, 576 placeholder tokens per
                  image, cycled.  Reports NON-PAD tokens/s of both.
Prints one JSON line per leg.
    python benchmarks/packed_micro.py --leg kernels [--rounds 10] [--iters 10] [--out FILE]
    python benchmarks/packed_micro.py --leg step [--micro-bsz 16] [--steps 3] [--grad-cp 0] [--out FILE]"""
import argparse
import json
import os
import random
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
            print(json.dumps({"bench": "packed_micro", "leg": self.what, "error": f"time limit of {self.seconds} s"}), flush=True)
            os._exit(124)
        signal.signal(signal.SIGALRM, stop)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def bench_layout(B, T, seed):
    rng = random.Random(seed)
    rows = []
    for _ in range(B):
        row, left = [], T
        while left > 0:
            n = min(16 * rng.randint(1, 60), left)
            row.append(n)
            left -= n
        rows.append(row)
    return rows


def leg_kernels(a):
    from benchmarks.wkv7_micro import synth_inputs
    from visualrwkv_amd import hip_lib
    from visualrwkv_amd.wkv7 import PackedLayout
    lib = hip_lib.load()
    B, T, H, dev = a.B, a.T, a.H, "cuda:0"
    w, q, k, v, z, aa, dy = synth_inputs(B, T, H, dev)
    y = torch.empty_like(v)
    s = torch.empty(B, H, T // 16, 64, 64, dtype=torch.float32, device=dev)
    sa = torch.empty(B, T, H, 64, dtype=torch.float32, device=dev)
    g = [torch.empty_like(w) for _ in range(6)]
    zero = torch.zeros(B, T // 16, dtype=torch.uint8, device=dev)
    rows = bench_layout(B, T, seed=B + T)
    lay = PackedLayout(rows, T, dev)
    st = torch.cuda.current_stream().cuda_stream
    P = lambda *ts: [t.data_ptr() for t in ts]

    def fwd_plain():
        assert lib.vrwkv_wkv7_forward_bf16(B, T, H, *P(w, q, k, v, z, aa, y, s, sa), st) == 0

    def fwd_packed(flags):
        return lambda: lib.vrwkv_wkv7_forward_packed_bf16(B, T, H, *P(w, q, k, v, z, aa, y, flags, s, sa), st)

    def bwd_plain():
        assert lib.vrwkv_wkv7_backward_bf16(B, T, H, *P(w, q, k, v, z, aa, dy, s, sa, *g), st) == 0

    def bwd_packed(flags):
        return lambda: lib.vrwkv_wkv7_backward_packed_bf16(B, T, H, *P(w, q, k, v, z, aa, dy, s, sa, flags, *g), st)

    def t(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters

    out = {"bench": "packed_micro", "leg": "kernels", "B": B, "T": T, "H": H, "rounds": a.rounds, "iters": a.iters,
           "segments_per_row_mean": round(sum(len(r) for r in rows) / B, 2), "device": torch.cuda.get_device_name(0)}
    for name, legs in (("fwd", [fwd_plain, fwd_plain, fwd_packed(zero), fwd_packed(lay.chunk_reset)]),
                       ("bwd", [bwd_plain, bwd_plain, bwd_packed(zero), bwd_packed(lay.chunk_reset)])):
        fwd_packed(lay.chunk_reset if name == "bwd" else zero)()          # the backward of a layout reads that layout's checkpoints
        for fn in legs * a.warmup:
            t(fn)
        times = [[] for _ in legs]
        for _ in range(a.rounds):
            if name == "bwd":
                # s / sa must match the flags of the backward that follows: regenerate them outside the timed region
                for i, fn in enumerate(legs):
                    (fwd_packed(lay.chunk_reset) if i == 3 else fwd_plain)()
                    times[i].append(t(fn))
            else:
                for i, fn in enumerate(legs):
                    times[i].append(t(fn))
        med = [statistics.median(x) for x in times]
        out[name] = {"plain_ms": round(med[0], 4), "plain_again_ms": round(med[1], 4), "packed_zero_flags_ms": round(med[2], 4),
                     "packed_layout_ms": round(med[3], 4), "plain_AA_rel": round(abs(med[1] - med[0]) / med[0], 4),
                     "plain_round_spread_rel": round((max(times[0] + times[1]) - min(times[0] + times[1])) / med[0], 4),
                     "zero_flags_over_plain": round(med[2] / med[0], 4), "layout_over_plain": round(med[3] / med[0], 4)}
    out["variants"] = {"fwd": lib.vrwkv_wkv7_last_variant(0), "bwd": lib.vrwkv_wkv7_last_variant(1)}
    return out


class ReplayTokenizer:
    """The recorded tokenisations of tests/golden/data_ref.pt (the reference's tokenizer is not shipped)."""

    def __init__(self, table):
        self.table = table

    def encode(self, text):
        return list(self.table[text])


def golden_samples(n_img_tokens, count):
    from visualrwkv_amd.data import build_sample
    gold = torch.load(os.path.join(ROOT, "tests", "golden", "data_ref.pt"), weights_only=False)
    tok = ReplayTokenizer(gold["token_table"])
    recs = gold["records"]
    out = []
    for i in range(count):
        r = dict(recs[i % len(recs)])
        px = {"dino": torch.zeros(1, 3, 448, 448), "siglip": torch.zeros(1, 3, 448, 448)}
        x = build_sample(r, tok, 1 << 20, n_img_tokens, pixel_values=px, do_pad_to_max_length=False)
        x["sample_id"] = f"{r['id']}#{i}"
        out.append(x)
    return out


def leg_step(a):
    import bench
    from visualrwkv_amd import build
    from visualrwkv_amd.data import multi_image_collate_fn, pack_batches, pad_to_max_len
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
    samples = golden_samples(576, a.samples)
    lens = [len(x["input_ids"]) for x in samples]

    def to_dev(b):
        out = {"input_ids": b["input_ids"].to(dev), "labels": b["labels"].to(dev), "sample_id": b["sample_id"]}
        out["images"] = {k: (v.to(dev, dtype=torch.bfloat16) if torch.is_tensor(v) else v) for k, v in b["images"].items() if k in towers or k == "num_image_per_sample"}
        for k in ("seg_lens", "n_samples"):
            if k in b:
                out[k] = b[k]
        return out

    padded = []
    for i in range(0, len(samples) - a.micro_bsz + 1, a.micro_bsz):
        rows = []
        for x in samples[i:i + a.micro_bsz]:
            ids, lab = pad_to_max_len(x["input_ids"], x["labels"], a.ctx_len, 0)
            row = dict(x, input_ids=ids, labels=lab)
            if "images" in x:                                # the collate of the reference wants all three towers' keys
                row["images"] = dict(x["images"], sam=torch.zeros(len(x["images"]["dino"]), 3, 8, 8))
            rows.append(row)
        padded.append(multi_image_collate_fn(rows))
    packed = list(pack_batches(samples, a.micro_bsz, a.ctx_len))

    def run(batches, what):
        n_tok, n_samp, times = 0, 0, []
        for i, b in enumerate(batches[:a.warmup + a.steps]):
            d = to_dev(b)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.zero_grad(set_to_none=True)
            loss = model.training_step(d)
            loss.backward()
            torch.cuda.synchronize()
            if i >= a.warmup:
                times.append(time.perf_counter() - t0)
                n_samp += b.get("n_samples", a.micro_bsz)
                ids = [s for row in b["sample_id"] for s in (row if isinstance(row, list) else [row])]
                n_tok += sum(min(lens[int(s.split("#")[1])], a.ctx_len) for s in ids)
        return {"what": what, "steps": len(times), "step_s_median": round(statistics.median(times), 4), "samples": n_samp, "non_pad_tokens": n_tok,
                "non_pad_tokens_per_s": round(n_tok / sum(times), 1), "row_tokens_per_s": round(len(times) * a.micro_bsz * a.ctx_len / sum(times), 1),
                "loss": round(float(loss.detach()), 4), "peak_GB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 1)}

    out = {"bench": "packed_micro", "leg": "step", "model": "1b5", "micro_bsz": a.micro_bsz, "ctx_len": a.ctx_len, "grad_cp": a.grad_cp,
           "sample_tokens_min_mean_max": [min(lens), round(sum(lens) / len(lens), 1), max(lens)], "device": torch.cuda.get_device_name(0),
           "note": "forward + backward, no optimizer step; both sides through the fused path"}
    out["padded"] = run(padded, "padded collate")
    torch.cuda.reset_peak_memory_stats()
    out["packed"] = run(packed, "pack_batches")
    out["samples_per_packed_batch"] = round(sum(b["n_samples"] for b in packed) / len(packed), 2)
    out["non_pad_speedup"] = round(out["packed"]["non_pad_tokens_per_s"] / out["padded"]["non_pad_tokens_per_s"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["kernels", "step"], required=True)
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--T", type=int, default=2624)
    ap.add_argument("--H", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--micro-bsz", type=int, default=16)
    ap.add_argument("--ctx-len", type=int, default=2624)
    ap.add_argument("--grad-cp", type=int, default=0)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--samples", type=int, default=256)
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
