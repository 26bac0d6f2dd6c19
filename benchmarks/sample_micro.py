"""The sampling head of the decode step (csrc/sample_head.hip), measured.
(a) the pick kernel alone at V = 65 536 for B = 1 and 4, against sampling.pick_torch on the GPU and against the device work of the greedy
    path's per-token tail (argmax, gather, softmax, gather): microseconds per call from HIP events around a batch of back-to-back calls, and
    the greedy tail once more with its three `.item()` read-backs, as generate_stateful runs it (wall clock).
(b) ms per generated token of the 1.5B stack: the sampled captured step (GraphDecoder.sample: copy of u, replay, one read-back) against the
    greedy loop of VisualRWKV.generate_stateful (argmax / gather / softmax with three `.item()`, emb, copy, replay), legs alternating in one
    process.  The greedy leg is the loop as it stands in visual.py, which sampling left untouched.
(c) presence / count penalties (vrwkv_sample_pick_pen_bf16): the plain and the penalised kernel alternated at B = 1 and 4 (occ with 256
    counted tokens per row), and per generated token, alternated with (b)'s legs: the penalised captured step
    (GraphDecoder(penalised=True)) and what the penalties cost without it -- the unsampled captured step, the penalties in torch on its
    logits, sampling.pick with the embedding row as x_out, the counts updated in torch, the embedding fed back (`penalised_by_hand`).
python benchmarks/sample_micro.py [n_tokens] [rounds]      one JSON line."""
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from visualrwkv_amd import sampling  # noqa: E402
from visualrwkv_amd.rwkv7 import RWKV  # noqa: E402

V, C = 65536, 2048


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def events_us(fn, calls=50, reps=9):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / calls)
    return spread(out)


def wall_us(fn, calls=50, reps=9):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6 / calls)
    return spread(out)


def kernel_leg(res):
    g = torch.Generator().manual_seed(0)
    emb = torch.randn(V, C, generator=g).bfloat16().cuda()
    for B in (1, 4):
        logits = (6 * torch.randn(B, V, generator=g)).bfloat16().cuda()
        u = torch.rand(B, generator=g).cuda()
        bufs = sampling.PickBuffers(B, logits.device)
        x_out = torch.empty(B, 1, C, device="cuda", dtype=torch.bfloat16)
        for name, (tau, top_p) in {"p0.9_t1": (1.0, 0.9), "p0.3_t0.7": (0.7, 0.3), "p1_t1": (1.0, 1.0), "p0_t1": (1.0, 0.0)}.items():
            bufs.set(tau, top_p)
            bufs.u.copy_(u)
            res[f"pick_kernel_us_B{B}_{name}"] = events_us(lambda: sampling.launch_pick(logits, bufs, emb, x_out))
        occ = torch.zeros(B, V, device="cuda")
        occ[:, torch.randperm(V, generator=g)[:256].cuda()] = 1.5
        bufs.set(1.0, 0.9, 0.4, 0.4, 0.996)
        pair = {"plain": [], "pen": []}
        for _ in range(5):                                   # alternated: the same clocks and neighbours for both
            pair["plain"].append(events_us(lambda: sampling.launch_pick(logits, bufs, emb, x_out), reps=3)["median"])
            pair["pen"].append(events_us(lambda: sampling.launch_pick(logits, bufs, emb, x_out, occ), reps=3)["median"])
        res[f"pick_kernel_alternated_us_B{B}"] = {k: spread(v) for k, v in pair.items()}
        res[f"pick_torch_us_B{B}"] = events_us(lambda: sampling.pick_torch(logits, 1.0, 0.9, u, emb, x_out), calls=10)

        def greedy_device():
            nxt = torch.argmax(logits, dim=-1, keepdim=True)
            return nxt, logits.gather(-1, nxt), torch.softmax(logits, dim=-1).gather(-1, nxt)
        res[f"greedy_tail_device_us_B{B}"] = events_us(greedy_device)
        if B == 1:
            def greedy_host():
                nxt = torch.argmax(logits, dim=-1, keepdim=True)
                return nxt.item(), logits.gather(-1, nxt).item(), torch.softmax(logits, dim=-1).gather(-1, nxt).item()
            res["greedy_tail_with_items_wall_us_B1"] = wall_us(greedy_host)

            def pick_host():
                sampling.launch_pick(logits, bufs, emb, x_out)
                return bufs.read()
            res["pick_with_readback_wall_us_B1"] = wall_us(pick_host)


def token_leg(res, n, rounds):
    args = SimpleNamespace(n_embd=C, n_layer=24, dim_att=C, head_size_a=64, head_size_divisor=8, vocab_size=V,
                           dropout=0, grad_cp=0, ctx_len=4096, load_model="", fused=True)
    torch.manual_seed(0)
    with torch.device("cuda"):
        m = RWKV(args)
    m = m.bfloat16().eval()
    prompt = torch.randn(1, 64, C, device="cuda", dtype=torch.bfloat16)
    with torch.no_grad():
        logits0, st = m.forward_stateful(prompt, None, last_only=True)
        greedy_dec = m.decoder_for(st)
        _, st2 = m.forward_stateful(prompt, None, last_only=True)
        sampled_dec = m.decoder_for(st2, sampled=True)
        sampled_dec.pick.set(1.0, 0.9)
        u_all = torch.rand(n, 1, device="cuda")

        def greedy(k):
            logits = logits0
            for _ in range(k):                               # VisualRWKV.generate_stateful's loop
                nxt = torch.argmax(logits, dim=-1, keepdim=True)
                nxt.item(); logits.gather(-1, nxt).item(); torch.softmax(logits, dim=-1).gather(-1, nxt).item()
                logits = greedy_dec(m.emb(nxt))

        def sampled(k):
            sampling.pick(logits0.contiguous(), 1.0, 0.9, u_all[0], m.emb.weight, sampled_dec.x_in)
            for i in range(k):
                sampled_dec.sample(u_all[i])

        _, st3 = m.forward_stateful(prompt, None, last_only=True)
        pen_dec = m.decoder_for(st3, sampled=True, penalised=True)
        pen_dec.pick.set(1.0, 0.9, 0.4, 0.4, 0.996)
        occ_hand = torch.zeros(1, V, device="cuda")
        nxt = torch.empty(1, 1, C, device="cuda", dtype=torch.bfloat16)

        def penalised(k):
            pen_dec.pick.reset()
            sampling.pick(logits0.contiguous(), 1.0, 0.9, u_all[0], m.emb.weight, pen_dec.x_in, pen_dec.pick.occ, 0.4, 0.4, 0.996)
            for i in range(k):
                pen_dec.sample(u_all[i])

        def penalised_by_hand(k):
            occ_hand.zero_()
            logits = logits0
            for i in range(k):
                l = torch.where(occ_hand > 0, (logits.float() - (0.4 + occ_hand * 0.4)).bfloat16(), logits)
                triple = sampling.pick(l, 1.0, 0.9, u_all[i], m.emb.weight, nxt)
                occ_hand.mul_(0.996)
                occ_hand[0, triple[0].long()] += 1.0
                [t.tolist() for t in triple]                 # the step's read-back, as generate_stateful's eager loop does it
                logits = greedy_dec(nxt)

        legs = {"greedy": greedy, "sampled": sampled, "penalised": penalised, "penalised_by_hand": penalised_by_hand}
        for fn in legs.values():
            fn(8)
        times = {k: [] for k in legs}
        for _ in range(rounds):
            for name, fn in legs.items():
                torch.cuda.synchronize(); t0 = time.perf_counter()
                fn(n)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3 / n)
        for name in legs:
            res[f"{name}_ms_per_token"] = spread(times[name])
        res["penalised_minus_sampled_ms_per_token"] = spread([b - a for a, b in zip(times["sampled"], times["penalised"])])


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    res = {"V": V, "C": C, "tokens_per_leg": n, "rounds": rounds}
    kernel_leg(res)
    token_leg(res, n, rounds)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
