"""RUN_CUDA_RWKV6_STATE / WKV_6_STATE and the v6.xx image-as-state model on the MI355X: the autograd op against fp64 autograd through the
oracle and against the fixture recorded from the reference's own recurrence, and the fused two-pass Block loop against the eager modules."""
import os
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn

from oracle.wkv7_oracle import rel_rms
from tests.test_wkv6_state import D_STATE0_TOL, G_TOL, GU_TOL, ST_TOL, Y_TOL, case

pytestmark = pytest.mark.gpu


def _op(ins, B, T, H, s0, gy=None, d_state_T=None, s_grad=True, want_state=True):
    from visualrwkv_amd import wkv6
    C = H * 64
    r, k, v, w = [ins[n].cuda().reshape(B, T, C).clone().requires_grad_(True) for n in ("r", "k", "v", "w")]
    u = ins["u"].cuda().clone().requires_grad_(True)
    s = s0.cuda().clone().requires_grad_(s_grad) if s0 is not None else None
    y, st = wkv6.RUN_CUDA_RWKV6_STATE(B, T, C, H, r, k, v, w, u, s, want_state)
    outs, grads = [], []
    if gy is not None:
        outs.append(y); grads.append(gy.cuda().reshape(B, T, C))
    if d_state_T is not None:
        outs.append(st); grads.append(d_state_T.cuda())
    torch.autograd.backward(outs, grads)
    torch.cuda.synchronize()
    g = [x.grad.cpu().view(B, T, H, 64) for x in (r, k, v, w)] + [u.grad.cpu(), s.grad.cpu() if s is not None and s.grad is not None else None]
    return y.detach().cpu().view(B, T, H, 64), st.detach().cpu() if st is not None else None, g


@pytest.fixture(scope="module")
def raw_case():
    """case() with the raw bf16 w beside ew"""
    from oracle.wkv6_oracle import make_inputs6

    def get(B, T, H):
        ins, ref = case(B, T, H)
        w = make_inputs6(B, T, H, seed=7000 + 10 * T + H)[3]
        assert torch.equal((-torch.exp(w.float())), ins["ew"])
        return dict(ins, w=w), ref
    return get


def _check(tag, ref, y, st, g, H, d0=True):
    figs = {"y": (rel_rms(y.double(), ref["y"]), Y_TOL), "state_T": (rel_rms(st.double(), ref["state_T"]), ST_TOL)}
    for n, o in zip(("gr", "gk", "gv", "gw"), g[:4]):
        figs[n] = (rel_rms(o.double(), ref[n]), G_TOL)
    figs["gu"] = (rel_rms(g[4].double(), ref["gu"]), GU_TOL["gpu"])
    if d0:
        figs["d_state0"] = (rel_rms(g[5].double(), ref["d_state0"]), D_STATE0_TOL)
    print(f"[wkv6 state op] {tag}: " + "  ".join(f"{n} {e:.3e}" for n, (e, _) in figs.items()))
    for n, (e, tol) in figs.items():
        assert e < tol, (tag, n, e, tol)


@pytest.mark.parametrize("B,T,H", [(2, 37, 3), (3, 129, 2)])
def test_op_matches_oracle(raw_case, B, T, H):
    ins, ref = raw_case(B, T, H)
    y, st, g = _op(ins, B, T, H, ins["s0"], ins["gy"], ins["dsT"])
    _check(f"{B}x{T}x{H}", ref, y, st, g, H)


def test_frozen_state_and_unused_final_state(raw_case, monkeypatch):
    """A frozen `s` asks the kernel for no d_state0; a final state that got no gradient (or was not requested) passes no d_state_T; the
    other gradients are those of the full call with d_state_T = 0."""
    from visualrwkv_amd import wkv6
    B, T, H = 2, 37, 3
    ins, _ = raw_case(B, T, H)
    seen = []
    real = wkv6.backward_hip

    def spy(*a, **kw):
        seen.append((kw.get("d_state_T") is not None, kw.get("d_state0") is not None))
        return real(*a, **kw)
    monkeypatch.setattr(wkv6, "backward_hip", spy)
    y0, st0, g0 = _op(ins, B, T, H, ins["s0"], ins["gy"], torch.zeros_like(ins["dsT"]))
    y1, st1, g1 = _op(ins, B, T, H, ins["s0"], ins["gy"], None, s_grad=False)
    y2, st2, g2 = _op(ins, B, T, H, ins["s0"], ins["gy"], None, want_state=False)
    assert seen == [(True, True), (False, False), (False, True)]
    assert g1[5] is None and st2 is None and torch.equal(st1, st0)
    assert torch.equal(y1, y0) and torch.equal(y2, y0)
    for a, b, c in zip(g0[:5], g1[:5], g2[:5]):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(g2[5], g0[5])
    # s = None is the zero state
    y3, st3, _ = _op(ins, B, T, H, None, ins["gy"])
    y4, st4, _ = _op(ins, B, T, H, torch.zeros_like(ins["s0"]), ins["gy"])
    assert torch.equal(y3, y4) and torch.equal(st3, st4)


def test_op_rejects_bad_states():
    from visualrwkv_amd import wkv6
    B, T, H = 1, 16, 2
    r = torch.zeros(B, T, 128, dtype=torch.bfloat16, device="cuda")
    u = torch.zeros(H, 64, dtype=torch.bfloat16, device="cuda")
    for bad in (torch.zeros(B, 1, 64, 64, device="cuda"), torch.zeros(B, H, 64, 32, device="cuda"), torch.zeros(B, H, 64, 64, device="cuda", dtype=torch.bfloat16)):
        with pytest.raises(ValueError):
            wkv6.RUN_CUDA_RWKV6_STATE(B, T, 128, H, r, r, r, r, u, bad)
    with pytest.raises(NotImplementedError):
        wkv6.RUN_CUDA_RWKV6_STATE(B, T, 128, H, r, r, r, r, u, torch.zeros(B, H, 64, 64))


def test_reference_recurrence_fixture_with_state():
    """The op on the `with_state` case of tests/golden/wkv6_naive_ref.pt -- the reference's own naive_recurrent_rwkv6_fla in fp64, autograd
    gradients of sum(y gy): y, final_state ([key][value] as recorded), the five gradients and gs0."""
    g = torch.load(os.path.join(os.path.dirname(__file__), "golden", "wkv6_naive_ref.pt"))
    B, T, H, N = g["B"], g["T"], g["H"], g["N"]
    c = g["with_state"]
    f = lambda x: x.view(B, T, H, N).bfloat16()
    ins = dict(r=f(g["r"]), k=f(g["k"]), v=f(g["v"]), w=f(g["w"]), u=g["u"].bfloat16())
    y, st, gr = _op(ins, B, T, H, c["s0"].float(), c["gy"].bfloat16())
    f4 = lambda x: x.view(B, T, H, N)
    ref = dict(y=f4(c["y"]), state_T=c["final_state"], gr=f4(c["gr"]), gk=f4(c["gk"]), gv=f4(c["gv"]), gw=f4(c["gw"]), gu=c["gu"], d_state0=c["gs0"])
    _check("reference fixture", ref, y, st, gr, H)


# ---------------------------------------------------------------------------------------------- the two-pass Block loop
def _args(fused, grad_cp):
    return SimpleNamespace(n_embd=128, dim_att=128, n_layer=2, head_size_a=64, head_size_divisor=8, dim_ffn=256, dropout=0, grad_cp=grad_cp,
                           vocab_size=64, fused=fused)


@pytest.fixture(scope="module")
def eager_runs():
    """The eager modules' run per (rows, T): computed once, shared by the grad_cp cases."""
    from visualrwkv_amd.rwkv6 import RWKV
    torch.manual_seed(3)
    ref = RWKV(_args(False, 0))
    proj = nn.Linear(32, 128, bias=False)
    with torch.no_grad():
        for p in ref.parameters():
            if float(p.abs().sum()) == 0.0:
                p.normal_(0, 0.05)
        for blk in ref.blocks:
            for ln in (blk.ln1, blk.ln2):
                ln.weight.normal_(1, 0.2); ln.bias.normal_(0, 0.1)
    ref, proj = ref.bfloat16().cuda(), proj.bfloat16().cuda()
    cache = {}

    def get(rows, T):
        if (rows, T) not in cache:
            g = torch.Generator(device="cuda").manual_seed(100 * rows + T)
            data = dict(x=(torch.randn(2, T, 128, device="cuda", generator=g) * 0.7).bfloat16(),
                        feats=torch.randn(2, rows, 32, device="cuda", generator=g).bfloat16(),
                        gy=torch.randn(2, T, 128, device="cuda", generator=g).bfloat16())
            cache[(rows, T)] = (data, _run(ref, proj, data))
        return cache[(rows, T)]
    return ref, proj, get


def _run(model, proj, data):
    model.zero_grad(set_to_none=True)
    proj.zero_grad(set_to_none=True)
    x = data["x"].clone().requires_grad_(True)
    h = model.forward_state(x, proj(data["feats"]))
    h.backward(data["gy"])
    torch.cuda.synchronize()
    grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    return h.detach(), x.grad.clone(), proj.weight.grad.clone(), grads


@pytest.mark.parametrize("grad_cp", [0, 1])
@pytest.mark.parametrize("rows,T", [(5, 24), (17, 40)])
def test_fused_two_pass_blocks_match_eager_modules(eager_runs, rows, T, grad_cp):
    """fused.blocks6_forward_state against RWKV.forward_state on the eager modules (both on the HIP op), C = 128: output, input gradient,
    every parameter gradient, and the projector's gradient -- which exists only through dL/dS.  Bounds of
    test_wkv6_gpu.py::test_fused_x060_glue_matches_eager_modules: 1e-2 / 2e-2 / 3e-2."""
    from visualrwkv_amd.rwkv6 import RWKV
    ref, proj, get = eager_runs
    data, (h0, gx0, gp0, g0) = get(rows, T)
    fus = RWKV(_args(True, grad_cp)).bfloat16().cuda()
    fus.load_state_dict(ref.state_dict())
    h1, gx1, gp1, g1 = _run(fus, proj, data)
    assert float(gp0.float().abs().max()) > 0 and float(gp1.float().abs().max()) > 0
    figs = {"h": (rel_rms(h1.float(), h0.float()), 1e-2), "gx": (rel_rms(gx1.float(), gx0.float()), 2e-2),
            "proj.weight": (rel_rms(gp1.float(), gp0.float()), 3e-2)}
    assert set(g0) == set(g1) and "blocks.0.att.key.weight" in g0
    for n in g0:
        figs[n] = (rel_rms(g1[n].float(), g0[n].float()), 3e-2)
    worst = max(figs.items(), key=lambda kv: kv[1][0] / kv[1][1])
    print(f"[v6 state fused] rows {rows} T {T} grad_cp {grad_cp}: h {figs['h'][0]:.2e} gx {figs['gx'][0]:.2e} proj {figs['proj.weight'][0]:.2e} worst {worst[0]} {worst[1][0]:.2e}")
    for n, (e, tol) in figs.items():
        assert e < tol, (n, e, tol)
