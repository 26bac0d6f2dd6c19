"""fused._HeadCE (head + loss, backward dense on the labelled rows only) against linear + _FusedCE on an MI355X, at the benchmark's shape
(16 x 2624 tokens, C 2048, V 65 536, bench.py's label mask) and at a padded T."""
import pytest
import torch

pytestmark = pytest.mark.gpu

V, C = 65536, 2048


def bench_labels(B, T, g):
    """bench.synthetic_batch's labels: ids with a run of 576 image placeholders (65535) after a 4-token prefix, -100 on the first 60 % and on
    the placeholders."""
    ids = torch.randint(0, 65535, (B, T), device="cuda", generator=g)
    ids[:, 4:4 + 576] = 65535
    labels = ids.clone()
    labels[:, : int(T * 0.6)] = -100
    labels[ids == 65535] = -100
    return labels


def run_both(B, T, labels, seed=0, xscale=1.0):
    from visualrwkv_amd import fused
    from visualrwkv_amd.rwkv7 import CHUNK_LEN
    g = torch.Generator(device="cuda").manual_seed(seed)
    pad = (CHUNK_LEN - T % CHUNK_LEN) % CHUNK_LEN
    head = torch.nn.Linear(C, V, bias=False, device="cuda", dtype=torch.bfloat16)
    with torch.no_grad():
        head.weight.copy_(torch.randn(V, C, device="cuda", generator=g) * 0.02)
    x0 = (torch.randn(B, T + pad, C, device="cuda", generator=g) * xscale).bfloat16()
    out = {}
    for mode in ("dense", "compact"):
        head.weight.grad = None
        x = x0.clone().requires_grad_(True)
        if mode == "dense":
            loss = fused.loss_from_logits(fused.linear(head, x)[:, pad:], labels, -100)
        else:
            plan = fused.HeadPlan(labels, pad)
            loss = fused.head_loss(head, x, plan)
            out["pos"] = plan.pos.view(B, T + pad)
        loss.backward()
        torch.cuda.synchronize()
        out[mode] = (loss.detach(), x.grad.detach(), head.weight.grad.detach().clone())
    return out


def rel_rms(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def check(out, tag):
    (l0, dx0, dw0), (l1, dx1, dw1) = out["dense"], out["compact"]
    pos = out["pos"]
    assert torch.equal(l0, l1), (tag, float(l0), float(l1))
    unl, lab, padr = pos == -1, pos >= 0, pos == -2
    assert torch.equal(dx1[unl], dx0[unl]), (tag, int((dx1[unl] != dx0[unl]).sum()))
    assert torch.equal(dx1[padr], torch.zeros_like(dx1[padr])) and torch.equal(dx0[padr], dx1[padr])
    r_dx, r_dw = rel_rms(dx1[lab], dx0[lab]), rel_rms(dw1, dw0)
    flips_dx, flips_dw = int((dx1[lab] != dx0[lab]).sum()), int((dw1 != dw0).sum())
    print(f"{tag}: loss {float(l0)} identical; labelled dx rel-RMS {r_dx:.2e} ({flips_dx} of {dx1[lab].numel()} differ), "
          f"dW rel-RMS {r_dw:.2e} ({flips_dw} of {dw1.numel()} differ)")
    assert r_dx <= 1e-3 and r_dw <= 1e-3, (tag, r_dx, r_dw)


def test_head_loss_matches_dense_at_bench_shape():
    g = torch.Generator(device="cuda").manual_seed(1)
    B, T = 16, 2624
    labels = bench_labels(B, T, g)
    check(run_both(B, T, labels), "16x2624")


def test_head_loss_matches_dense_at_padded_T():
    g = torch.Generator(device="cuda").manual_seed(2)
    B, T = 4, 2615                                 # T % 16 = 7: 9 pad rows per sample
    labels = bench_labels(B, T, g)
    labels[1] = -100                               # a sample without labels
    check(run_both(B, T, labels, seed=3), "4x2615")


def test_dense_fallback_above_threshold_is_the_old_path():
    """All rows labelled: the node's backward is linear + _FusedCE's, bit for bit."""
    g = torch.Generator(device="cuda").manual_seed(4)
    B, T = 2, 1024
    labels = torch.randint(0, V, (B, T), device="cuda", generator=g)
    out = run_both(B, T, labels, seed=5)
    for a, b in zip(out["dense"], out["compact"]):
        assert torch.equal(a, b)


def test_compact_backward_is_deterministic():
    from visualrwkv_amd import fused
    g = torch.Generator(device="cuda").manual_seed(6)
    B, T = 2, 2624
    labels = bench_labels(B, T, g)
    head = torch.nn.Linear(C, V, bias=False, device="cuda", dtype=torch.bfloat16)
    x0 = torch.randn(B, T, C, device="cuda", generator=g).bfloat16()
    grads = []
    for _ in range(2):
        head.weight.grad = None
        x = x0.clone().requires_grad_(True)
        fused.head_loss(head, x, fused.HeadPlan(labels, 0)).backward()
        grads.append((x.grad.view(torch.int16).clone(), head.weight.grad.view(torch.int16).clone()))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
