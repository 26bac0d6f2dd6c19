"""The head's backward on labelled rows only (csrc/loss_fused.hip: ce_bwd_rows, head_dx, l2wrap_wgrad; fused._HeadCE) through the host
lockstep emulator, at small V and C, against the dense backward of linear + _FusedCE: the full (rows, V) logit gradient of ce_bwd, then
dx = dlogits W and dW = dlogits^T x in fp32 with one bf16 rounding (what the library GEMMs compute).  No GPU needed."""
import ctypes

import numpy as np
import pytest
import torch

L, I, F32, VP = ctypes.c_long, ctypes.c_int, ctypes.c_float, ctypes.c_void_p
U = 2.0 ** -8            # bf16 unit round-off


def P(t):
    return VP(t.data_ptr()) if t is not None else VP(0)


def call(lib, name, argtypes, *args):
    f = getattr(lib, name)
    f.argtypes, f.restype = argtypes, I
    rc = f(*args)
    assert rc == 0, (name, rc)


def ce_fwd(lib, logits, labels):
    n, V = logits.shape
    loss, mx, lse = torch.zeros(n), torch.zeros(n), torch.zeros(n)
    arg = torch.zeros(n, dtype=torch.int32)
    call(lib, "vrwkv_ce_fwd_bf16", [L, I] + [VP] * 7, n, V, P(logits), P(labels), P(loss), P(mx), P(lse), P(arg), None)
    return loss, mx, lse, arg


def ce_bwd_dense(lib, logits, labels, row_w, mx, lse, arg, l2f):
    d = torch.zeros_like(logits)
    call(lib, "vrwkv_ce_bwd_bf16", [L, I] + [VP] * 6 + [F32, VP, VP], logits.shape[0], logits.shape[1], P(logits), P(labels), P(row_w),
         P(mx), P(lse), P(arg), l2f, P(d), None)
    return d


def ce_bwd_rows(lib, logits, labels, row_w, mx, lse, arg, l2f, idx):
    d = torch.full((idx.numel(), logits.shape[1]), 7.0).bfloat16()          # garbage: every row must be written
    call(lib, "vrwkv_ce_bwd_rows_bf16", [L, I] + [VP] * 6 + [F32, VP, VP, VP], idx.numel(), logits.shape[1], P(logits), P(labels), P(row_w),
         P(mx), P(lse), P(arg), l2f, P(idx), P(d), None)
    return d


def head_dx(lib, pos, dxc, W, mx, arg, l2f):
    dx = torch.full((pos.numel(), W.shape[1]), 7.0).bfloat16()
    call(lib, "vrwkv_head_dx_bf16", [L, I] + [VP] * 5 + [F32, VP, VP], pos.numel(), W.shape[1], P(pos), P(dxc), P(W), P(mx), P(arg), l2f,
         P(dx), None)
    return dx


def l2wrap_wgrad(lib, srow, x, mx, arg, l2f, dW):
    n, C = srow.numel(), x.shape[1]
    f = lib.vrwkv_l2wrap_wgrad_ws_floats
    f.argtypes, f.restype = [L, I], L
    ws = torch.full((max(f(n, C), 1),), float("nan"))
    call(lib, "vrwkv_l2wrap_wgrad_bf16", [L, I] + [VP] * 4 + [F32, VP, VP, VP], n, C, P(srow), P(x), P(mx), P(arg), l2f, P(dW), P(ws), None)


def gemm(a, b):
    """a @ b of bf16 operands, fp32 accumulation, one bf16 rounding (the library GEMM's arithmetic)."""
    return (a.float() @ b.float()).bfloat16()


def bf16_coef(mx, l2f):
    return (mx * np.float32(l2f)).bfloat16().float()


def make_case(B, T, pad, C, V, label_rows, seed, tie_rows=(), shared_arg_rows=()):
    """Hidden state x (B*(T+pad), C), head W (V, C), logits, and the shifted labels in the padded layout (label_rows: per sample the
    real positions that carry a label); tie_rows get two equal maxima, shared_arg_rows one common arg-max."""
    g = torch.Generator().manual_seed(seed)
    Tp = T + pad
    x = torch.randn(B * Tp, C, generator=g).bfloat16()
    W = (0.5 * torch.randn(V, C, generator=g)).bfloat16()
    logits = gemm(x, W.t())
    for r in tie_rows:
        m = logits[r].float().max() + 1.0
        logits[r, 5] = m
        logits[r, 3] = m                                  # the lower index wins
    for r in shared_arg_rows:
        logits[r, V - 3] = logits[r].float().max() + 2.0
    labels = torch.full((B, Tp), -100, dtype=torch.long)
    for b, rows in enumerate(label_rows):
        for t in rows:
            labels[b, pad + t] = int(torch.randint(0, V, (1,), generator=g))
    real = torch.zeros(B, Tp, dtype=torch.bool)
    real[:, pad:] = True
    return x, W, logits, labels.view(-1), real.view(-1)


def compact_backward(lib, x, W, logits, labels, real, row_w, l2f, align):
    """fused._HeadCE.backward's compact branch with torch GEMMs on the host."""
    N, C = x.shape
    V = W.shape[0]
    _, mx, lse, arg = ce_fwd(lib, logits, labels)
    mask = labels >= 0
    n_lab = int(mask.sum())
    nrows = -(-n_lab // align) * align
    order = torch.argsort((~mask).to(torch.int8), stable=True)
    idx = torch.full((nrows,), -1, dtype=torch.long)
    idx[:n_lab] = order[:n_lab]
    pos = torch.where(mask, torch.cumsum(mask, 0) - 1, torch.where(real, -1, -2))
    dlog = ce_bwd_rows(lib, logits, labels, row_w, mx, lse, arg, l2f, idx) if nrows else torch.zeros(0, V).bfloat16()
    dxc = gemm(dlog, W) if nrows else torch.zeros(0, C).bfloat16()
    dx = head_dx(lib, pos, dxc, W, mx, arg, l2f)
    dW = gemm(dlog.t(), x.index_select(0, idx.clamp(min=0))) if nrows else torch.zeros(V, C).bfloat16()
    dW_gemm = dW.clone()
    n_u = int((pos == -1).sum())
    if n_u:
        key = torch.where(pos == -1, arg.long(), V)
        srow = torch.sort(key, stable=True).indices[:n_u].contiguous()
        l2wrap_wgrad(lib, srow, x, mx, arg, l2f, dW)
    return dict(dlog=dlog, idx=idx, pos=pos, dx=dx, dW=dW, dW_gemm=dW_gemm, mx=mx, lse=lse, arg=arg)


def dense_backward(lib, x, W, logits, labels, real, row_w, l2f):
    _, mx, lse, arg = ce_fwd(lib, logits, labels)
    dlog = ce_bwd_dense(lib, logits, labels, row_w, mx, lse, arg, l2f)
    dlog[~real] = 0                                        # pad rows: unpad's backward gives them no gradient
    return dict(dlog=dlog, dx=gemm(dlog, W), dW=gemm(dlog.t(), x), arg=arg, mx=mx)


def rows_weight(labels, real, B):
    lab = labels.view(B, -1)
    valid = (lab >= 0).sum(1).clamp(min=1)
    return ((lab >= 0).float() / (valid.float().unsqueeze(1) * B)).view(-1) * real.float()


CASES = {
    # name: B, T, pad, C, V, labelled positions per sample, tie rows, shared-arg rows
    "mixed_padded": (2, 37, 3, 64, 256, [range(20, 36), range(30, 36)], (3, 50), (4, 6, 9, 44, 45, 46)),
    "no_labels_in_one_sample": (2, 40, 0, 64, 256, [[], range(10, 39)], (1,), (0, 2, 5)),
    "all_labelled_sample": (2, 24, 8, 32, 128, [range(0, 23), [5]], (), (40, 41)),
    "no_labels_at_all": (1, 48, 0, 64, 256, [[]], (7,), (1, 2, 3)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_compact_backward_matches_dense(emu_lib, name):
    B, T, pad, C, V, lab_rows, ties, shared = CASES[name]
    x, W, logits, labels, real = make_case(B, T, pad, C, V, lab_rows, seed=len(name), tie_rows=ties, shared_arg_rows=shared)
    row_w = rows_weight(labels, real, B)
    l2f = 1e-4 / (B * T)
    c = compact_backward(emu_lib, x, W, logits, labels, real, row_w, l2f, align=16)
    d = dense_backward(emu_lib, x, W, logits, labels, real, row_w, l2f)
    lab = labels >= 0
    unl = real & ~lab
    # argmax ties: the lower index, as ce_fwd; shared arg-max rows really share it
    for r in ties:
        assert int(c["arg"][r]) == 3
    if shared:
        assert len({int(c["arg"][r]) for r in shared}) == 1
    # compact CE rows are the dense rows, bit for bit; padding rows of the compact matrix are zeros
    n_lab = int(lab.sum())
    assert torch.equal(c["dlog"][:n_lab], d["dlog"][c["idx"][:n_lab]])
    assert torch.equal(c["dlog"][n_lab:], torch.zeros_like(c["dlog"][n_lab:]))
    # a row without a label: one nonzero logit gradient bf16(max * l2f) at the arg-max
    rows = unl.nonzero().flatten()
    if rows.numel():
        coef = bf16_coef(d["mx"][rows], l2f)
        dl = d["dlog"][rows].float()
        assert torch.equal(dl[torch.arange(rows.numel()), d["arg"][rows].long()], coef)
        assert int((dl != 0).sum()) == int((coef != 0).sum())
    # dx: unlabelled rows bit-identical to the dense GEMM, labelled rows the same GEMM rows, pad rows zero
    assert torch.equal(c["dx"][unl], d["dx"][unl])
    assert torch.equal(c["dx"][lab], d["dx"][lab])
    assert torch.equal(c["dx"][~real], torch.zeros_like(c["dx"][~real]))
    # dW: the labelled rows' GEMM + the sparse rows, against the exact sum, within the double-rounding bound of DESIGN.md
    exact = d["dlog"].double().t() @ x.double()
    G = c["dW_gemm"].double()
    absprod = d["dlog"].double().abs().t() @ x.double().abs()
    bound = 1.01 * U * (G.abs() + exact.abs()) + 1e-5 * absprod
    assert bool(((c["dW"].double() - exact).abs() <= bound).all())
    rel = float((c["dW"].double() - d["dW"].double()).norm() / exact.norm().clamp_min(1e-30))
    assert rel < 1e-2


def test_sparse_weight_gradient_groups_and_determinism(emu_lib):
    """Runs of one arg-max longer than a tile, a run ending exactly at a tile end, single rows; against fp64 and repeatable bit for bit."""
    g = torch.Generator().manual_seed(11)
    n_rows, C, V = 300, 64, 64
    x = torch.randn(n_rows, C, generator=g).bfloat16()
    mx = (10 * torch.rand(n_rows, generator=g) - 2)
    arg = torch.cat([torch.full((100,), 7), torch.full((28,), 9), torch.full((1,), 10), torch.full((3,), 11),
                     torch.randint(12, V, (168,), generator=g)]).to(torch.int32)
    arg = arg[torch.randperm(n_rows, generator=g)].contiguous()
    l2f = 1e-2
    srow = torch.sort(arg.long(), stable=True).indices[:250].contiguous()      # the first 250 of the sorted list (the rest: "labelled")
    base = (0.01 * torch.randn(V, C, generator=g)).bfloat16()
    outs = []
    for _ in range(2):
        dW = base.clone()
        l2wrap_wgrad(emu_lib, srow, x, mx, arg, l2f, dW)
        outs.append(dW)
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    coef = bf16_coef(mx, l2f).double()
    S = torch.zeros(V, C, dtype=torch.float64)
    S.index_add_(0, arg[srow].long(), coef[srow, None] * x[srow].double())
    G = base.double()
    err = (outs[0].double() - (G + S)).abs()
    tol = U * (G.abs() + (G + S).abs()) + 1e-6 * (coef[srow].abs().max() * x.double().abs().max())
    assert bool((err <= tol).all())
    untouched = torch.ones(V, dtype=torch.bool)
    untouched[arg[srow].long()] = False
    assert torch.equal(outs[0][untouched], base[untouched])
