"""The one-token RWKV-6 decode kernels -- csrc/wkv6_step.hip (the WKV6 state step), csrc/decode6_fused.hip (ddlerp, tmix6_head) and the
gated entry of csrc/gemv_decode.hip -- through the C ABI, on two backends with the same test bodies: the host lockstep emulator
(tests/emu/emu_decode6.cpp and emu_gemv_decode.cpp compile the .hip files whole: CPU tensors, no marker) and the product library (CUDA
tensors, `gpu` marker).

References: plain torch in fp64 on the backend's device, written from RWKV_Tmix_x060 / RWKV_CMix_x060 of the reference
(VisualRWKV-v6/v6.0/src/model.py:92-226, the carried state of v6.xx/src/model.py:137-144), with a bf16 rounding wherever the module path
holds a bf16 tensor.
  step       oracle.wkv6_oracle.wkv6_naive(..., state0) at T = 1 in fp64 (its state is [value][key]: the transpose of the kernels')
  ddlerp     out_j = h + (x_prev - h) (maa_j + hid_j w2_j[:, c]), rounded once
  tmix6_head lo = bf16(hid w2), w_raw = bf16(lo + time_decay), the step with u = time_faaaa, y = bf16, gn = bf16(GroupNorm(y)),
             sg = bf16(silu(g)), out = gn sg
  gated GEMV res + gate act(x W^T), rounded once
Every case asserts: return code 0; outputs are NaN before the call and every output buffer ends in a guard row -- results finite, guards
untouched; a second call on the same inputs is bit-identical.  The rejections assert the exact VRWKV_E* code and that outputs, the state
and the carried row are untouched.

Bounds.
  Single roundings (the step's y, ddlerp's rows, the gated GEMV): tests.parity.bf16_close against the reference rounded once, tol 1e-3,
  flips < 0.01 (FLIP_Y of the project).  The step's fp32 state after three chained steps: rel-RMS 2e-6, the bound tests/test_decode_shapes.py
  holds wkv7_step's fp32 state to (two 1-ulp exponentials and one FMA per step: about 2e-7 each).
  The step chain against vrwkv_wkv6_forward_state_bf16 at T = 16 (test_step_layout): the state op's own bounds in tests/test_wkv6_state.py,
  3e-3 for y and 2e-5 for state_T, on both sides of the comparison.
  Chains with intermediate roundings (tmix6_head's out and fp32 state): rel-RMS against the fp64 chain, test_decode_shapes.py's rule.  The
  floor is the same staged reference in fp32 torch, and again with every exp and rsqrt result moved up one fp32 ulp, against the fp64 one,
  on the CPU, worst over all cases; the bound is 4 x that floor, capped by what tests/test_stateful_gpu.py asserts (1e-2 output, 2e-3 state).
  VRWKV_TEST_NOTES=1 prints every figure, the floors included.
  Floors (worst case of the fp32 staged reference | of the same with nudged exp / rsqrt), the bound, the worst kernel figure:
    tmix6 out    2.346e-04 | 2.346e-04 (B4H64-D128; 0 in the three smaller cases)  ->  9.4e-4    emulator 2.346e-04 (B4H64-D128), MI355X 5.108e-05 (B4H64-D128)
    tmix6 state  2.806e-08 | 3.624e-08 (B2H2-D128)                                ->  1.45e-7   emulator 2.610e-08 (B4H64-D128), MI355X 2.638e-08 (B3H5-D64)
  (Each backend draws its inputs from its own device's generator, so the two columns are not the same data.)
  Single roundings, worst flips: emulator 1.3e-4 (ddlerp C1024-D64-B3), MI355X 2.4e-4 (step B4H64, second and third step).  The step's fp32
  state after three steps: 4.2e-8 / 4.6e-8; the decay of the k = 0 head per key row: at most 1.5e-7 / 1.9e-7 against the 2e-6 asserted
  for every row.
  test_step_layout, y | state_T: emulator 8.9e-5 | 2.1e-6, MI355X 2.4e-4 | 2.0e-6.
  The out floor is ties of intermediate bf16 roundings (every element of the three smaller cases is the rounded reference), so it is
  spiky; the state's is fp32 arithmetic alone: no rounding to bf16 lies between the inputs and the state but w_raw's, and lo, w_raw and y
  come from fp32 FMAs in the kernel's fixed order, the same bits on both backends.
  What a rel-RMS bound cannot see in the decay is asserted per key row on a head with k = 0, and a transposed state cannot pass
  test_step_layout (one-hot k, ramp v).
"""
import pytest
import torch

from oracle.wkv6_oracle import wkv6_naive
from tests.parity import NOTES, group_bias
from tests.shape_checks import Checks
from tests.test_glue_shapes import F32, I, L, P, VP, Backend, bits, nan_rows, rnd, same_bits, unif, written

EPS_GN = 64e-5                                  # 1e-5 head_size_divisor^2, head_size_divisor = 8
TOL = 1e-3
FLIP = {"emu": 0.01, "hip": 0.01}              # the project's limit for a result that is rounded once (FLIP_Y)
STEP_STATE = 2e-6
Y_TOL, ST_TOL = 3e-3, 2e-5                      # tests/test_wkv6_state.py
CHAIN = {"tmix6_out": 9.4e-4, "tmix6_state": 1.45e-7}      # 4 x the worst floor (module docstring)
CHAIN_CAP = {"tmix6_out": 1e-2, "tmix6_state": 2e-3}       # tests/test_stateful_gpu.py
EINVAL, ESHAPE, EALIGN = -1, -2, -3

BACKENDS = ["emu", pytest.param("hip", marks=pytest.mark.gpu)]
STEP_BH = [(1, 1), (3, 5), (4, 64)]
DDLERP_C = [64, 256, 1024, 4096, 8192]          # 1024: 1000 rounded to the next multiple of 64
HEAD_CASES = [(1, 1, 64), (3, 5, 64), (2, 2, 128), (4, 64, 128)]
GATED = [("short", 96, (1, 8, 9, 33, 70)), ("long", 520, (1, 7, 9, 17)), ("split", 2080, (1, 2, 3, 5))]      # K < 512 | K >= 512 | K > 2048

CHECKS = Checks("decode6", FLIP, {"emu": 0.0, "hip": 0.0}, TOL)
WORST = {}


def _params(items):
    out = []
    for b in BACKENDS:
        name, marks = (b, ()) if isinstance(b, str) else (b.values[0], b.marks)
        for it in items:
            it = it if isinstance(it, tuple) else (it,)
            out.append(pytest.param(name, *it, id="-".join(str(v) for v in (name,) + it), marks=marks))
    return out


@pytest.fixture
def be(request, backend):
    return Backend(request, backend)


def rc_of(be, fn, argtypes, *args):
    f = getattr(be.lib, fn)
    f.argtypes, f.restype = argtypes + [VP], I
    return f(*args, be.stream)


def arr(ts):
    """Pointer array; an int is taken as an address, None as NULL."""
    return (VP * len(ts))(*[t if isinstance(t, int) else t.data_ptr() if t is not None else 0 for t in ts])


def ints(vs):
    return (I * len(vs))(*vs)


def rel_rms(x, ref):
    x, ref = x.double().cpu().reshape(-1), ref.double().cpu().reshape(-1)
    return float((x - ref).norm() / ref.norm().clamp_min(1e-300))


def rb64(t):
    return t.float().bfloat16().to(t.dtype)


def nan_state(be, n):
    """n state tiles to be updated in place plus one guard tile, all NaN."""
    return torch.full((n + 1, 64, 64), float("nan"), dtype=torch.float32, device=be.dev)


class Ops:
    """The arithmetic of a staged reference: fp64, or fp32 with (nudge) every exp / rsqrt result one ulp up, for the floors."""
    def __init__(self, dt=torch.float64, nudge=False):
        self.dt, self.nudge = dt, nudge

    def t(self, x):
        return x.to(self.dt)

    def up(self, x):
        return torch.nextafter(x, torch.full_like(x, float("inf"))) if self.nudge else x

    def exp(self, x):
        return self.up(torch.exp(x))

    def rsqrt(self, x):
        return self.up(torch.rsqrt(x))

    def rb(self, x):
        return x.float().bfloat16().to(self.dt)


O64 = Ops()


def chain(be, kind, got, ref, name):
    """A result behind intermediate roundings: rel-RMS against the fp64 chain (rounded once where the result is bf16)."""
    ref = ref.detach()
    if got.dtype == torch.bfloat16:
        ref = rb64(ref)
    err = rel_rms(got, ref)
    key = (be.name, kind)
    if err > WORST.get(key, (0.0, ""))[0]:
        WORST[key] = (err, name)
    if NOTES:
        print(f"[decode6] {be.name} {name}: {kind} rel-RMS {err:.3e}   (worst so far {WORST[key][0] if key in WORST else 0.0:.3e})")
    assert CHAIN[kind] <= CHAIN_CAP[kind]
    assert err < CHAIN[kind], f"{name}: {kind} rel-RMS {err:.3e} >= {CHAIN[kind]:.1e}"


# ------------------------------------------------------------------------------------------------ wkv6 step
STEP_ARGT = [I, I] + [VP] * 7


def step_inputs(be, g, B, H, n):
    """n tokens: r, k, v ~ N(0, 0.5^2), w_raw ~ U(-8, 1) (the reference's own kernel test), u ~ N(0, 0.3^2)."""
    toks = [dict(r=rnd(be, g, B, H, 64, scale=0.5), k=rnd(be, g, B, H, 64, scale=0.5), v=rnd(be, g, B, H, 64, scale=0.5),
                 w=(torch.rand(B, H, 64, generator=g, device=be.dev) * 9 - 8).bfloat16()) for _ in range(n)]
    return toks, rnd(be, g, H, 64, scale=0.3)


def run_step(be, B, H, t, u, S):
    """One launch on a copy of S (B,H,64,64) -> (y (B H + 1, 64) with its guard row, the state tiles with their guard tile)."""
    state = nan_state(be, B * H)
    state[:-1] = S.reshape(B * H, 64, 64)
    y = nan_rows(be, B * H, 64)
    be.call("vrwkv_wkv6_step_bf16", STEP_ARGT, B, H, P(t["r"]), P(t["k"]), P(t["v"]), P(t["w"]), P(u), P(state), P(y))
    res = {"y": y, "state": state}
    written(res, None, 0)
    return res


@pytest.mark.parametrize("backend,B,H", _params(STEP_BH))
def test_step(backend, be, B, H):
    """Three steps chained, each against the oracle at T = 1 from the oracle's own state."""
    g = be.gen(100 * B + H)
    toks, u = step_inputs(be, g, B, H, 3)
    S = torch.randn(B, H, 64, 64, generator=g, device=be.dev) * 0.3
    S_ref = S.double().transpose(-1, -2)                                        # the oracle's [value][key]
    for n, t in enumerate(toks):
        res = run_step(be, B, H, t, u, S)
        if n == 0:
            same_bits(res, run_step(be, B, H, t, u, S))
        y_ref, S_ref = wkv6_naive(*[t[x].double().unsqueeze(1) for x in ("r", "k", "v", "w")], u.double(), state0=S_ref)
        CHECKS.act(be, res["y"], y_ref[:, 0].reshape(B * H, 64), f"step/B{B}H{H} y{n}")
        S = res["state"][:-1].view(B, H, 64, 64).clone()
        err = rel_rms(S, S_ref.transpose(-1, -2))
        if NOTES:
            print(f"[decode6] {be.name} step/B{B}H{H} state after step {n}: rel-RMS {err:.3e}")
        assert err < STEP_STATE, (n, err)
    group_bias(res["y"][:-1], y_ref[:, 0].reshape(B * H, 64), f"step/B{B}H{H}")


@pytest.mark.parametrize("backend", _params([()]))
def test_step_layout(backend, be):
    """16 steps from zeros and 16 more from a random state against vrwkv_wkv6_forward_state_bf16 at T = 16 on the same rows: y and state_T
    within the state op's own bounds.  k is one-hot (key index 5 t + 3 h + b, mod 64) and v a ramp, so S is far from symmetric: a
    transposed state gives other numbers in both."""
    B, H, T = 2, 2, 16
    g = be.gen(616)
    toks, u = step_inputs(be, g, B, H, T)
    ramp = ((torch.arange(64, device=be.dev, dtype=torch.float32) + 1) / 64)
    for n, t in enumerate(toks):
        k = torch.zeros(B, H, 64, device=be.dev)
        for b in range(B):
            for h in range(H):
                k[b, h, (5 * n + 3 * h + b) % 64] = 1.0 + 0.25 * h
        t["k"] = k.bfloat16()
        t["v"] = (ramp * (1 + 0.125 * n)).expand(B, H, 64).bfloat16().contiguous()
    fwd = be.lib.vrwkv_wkv6_forward_state_bf16
    fwd.argtypes, fwd.restype = [I] * 4 + [VP] * 10, I
    stack = lambda x: torch.stack([t[x] for t in toks], dim=1).contiguous()      # (B,T,H,64)
    r, k, v, w = stack("r"), stack("k"), stack("v"), stack("w")
    ew = (-torch.exp(w.float())).contiguous()
    for tag, S0 in (("zeros", torch.zeros(B, H, 64, 64, device=be.dev)), ("random", torch.randn(B, H, 64, 64, generator=g, device=be.dev) * 0.3)):
        y_op, sT = torch.zeros_like(r), torch.zeros(B, H, 64, 64, device=be.dev)
        ck = torch.zeros(B * H, 1, 64, 64, device=be.dev)
        assert fwd(B, T, H * 64, H, P(r), P(k), P(v), P(ew), P(u), P(S0), P(y_op), P(sT), P(ck), be.stream) == 0
        S, ys = S0.clone(), []
        for t in toks:
            res = run_step(be, B, H, t, u, S)
            S = res["state"][:-1].view(B, H, 64, 64).clone()
            ys.append(res["y"][:-1].view(B, H, 64))
        y_steps = torch.stack(ys, dim=1)
        ey, es = rel_rms(y_steps, y_op), rel_rms(S, sT)
        if NOTES:
            print(f"[decode6] {be.name} step_layout/{tag}: y rel-RMS {ey:.3e}, state_T rel-RMS {es:.3e}")
        assert ey < Y_TOL and es < ST_TOL, (tag, ey, es)
        assert rel_rms(S.transpose(-1, -2), sT) > 0.5, "the data cannot tell a transposed state"
        # and both against the oracle
        y_ref, S_ref = wkv6_naive(r.double(), k.double(), v.double(), w.double(), u.double(), state0=S0.double().transpose(-1, -2))
        assert rel_rms(y_steps, y_ref) < Y_TOL and rel_rms(S, S_ref.transpose(-1, -2)) < ST_TOL


# ------------------------------------------------------------------------------------------------ ddlerp
DD_ARGT = [I, I, I] + [VP] * 6


def run_ddlerp(be, B, C, D, h, prev, hid, w2, maa):
    carried = nan_rows(be, B, C)
    carried[:-1] = prev
    outs = [nan_rows(be, B, C) for _ in range(5)]
    be.call("vrwkv_decode6_ddlerp_bf16", DD_ARGT, B, C, D, P(h), P(carried), P(hid), P(w2), arr(maa), arr(outs))
    res = {"x_prev": carried, **{f"out{j}": o for j, o in enumerate(outs)}}
    written(res, None, 0)
    return res


@pytest.mark.parametrize("backend,C,D,B", _params([(C, D, B) for C in DDLERP_C for D in (32, 64) for B in (1, 3, 4)]))
def test_ddlerp(backend, be, C, D, B):
    g = be.gen(C + 7 * D + B)
    h, prev = rnd(be, g, B, C), rnd(be, g, B, C)
    hid = torch.tanh(torch.randn(B, 5 * D, generator=g, device=be.dev)).bfloat16()
    w2 = rnd(be, g, 5, D, C, scale=D ** -0.5)
    maa = [unif(be, g, C) for _ in range(5)]
    res = run_ddlerp(be, B, C, D, h, prev, hid, w2, maa)
    same_bits(res, run_ddlerp(be, B, C, D, h, prev, hid, w2, maa))
    assert torch.equal(bits(res["x_prev"][:-1]), bits(h)), "x_prev is not h"
    m = torch.bmm(hid.double().view(B, 5, D).transpose(0, 1), w2.double())       # (5,B,C)
    got, want = [], []
    for j in range(5):
        got.append(res[f"out{j}"][:-1].reshape(-1))
        want.append((h.double() + (prev.double() - h.double()) * (maa[j].double() + m[j])).reshape(-1))
    CHECKS.act(be, torch.cat(got), torch.cat(want), f"ddlerp/C{C}-D{D}-B{B}", guard=False)
    group_bias(torch.cat(got), torch.cat(want), f"ddlerp/C{C}-D{D}-B{B}")


# ------------------------------------------------------------------------------------------------ tmix6_head
HEAD_ARGT = [I, I, I] + [VP] * 10 + [F32] + [VP] * 2


def head_inputs(be, g, B, H, Dd):
    C = H * 64
    p = dict(B=B, H=H, Dd=Dd)
    p["r"], p["k"], p["v"] = [rnd(be, g, B, C, scale=0.5) for _ in range(3)]
    p["g"] = rnd(be, g, B, C)
    p["hid"] = torch.tanh(torch.randn(B, Dd, generator=g, device=be.dev)).bfloat16()
    p["w2"] = rnd(be, g, Dd, C, scale=Dd ** -0.5)
    p["td"] = rnd(be, g, C, scale=1.5, shift=-3.0)                              # time_decay is -6 .. -1 at initialisation
    p["u"] = rnd(be, g, C, scale=0.3)
    p["ln_w"], p["ln_b"] = rnd(be, g, C, scale=0.2, shift=1.0), rnd(be, g, C, scale=0.1)
    p["S"] = torch.randn(B, H, 64, 64, generator=g, device=be.dev) * 0.1
    return p


def run_head(be, p):
    B, H = p["B"], p["H"]
    state = nan_state(be, B * H)
    state[:-1] = p["S"].view(B * H, 64, 64)
    out = nan_rows(be, B, H * 64)
    be.call("vrwkv_decode6_tmix_head_bf16", HEAD_ARGT, B, H, p["Dd"], P(p["r"]), P(p["k"]), P(p["v"]), P(p["g"]), P(p["hid"]), P(p["w2"]),
            P(p["td"]), P(p["u"]), P(p["ln_w"]), P(p["ln_b"]), EPS_GN, P(state), P(out))
    res = {"out": out, "state": state}
    written(res, None, 0)
    return res


def head_ref(o, p):
    """-> out (B,C), the new state (B,H,64,64) [key][value], w_raw (B,H,64)."""
    B, H = p["B"], p["H"]
    t, hd = o.t, lambda x: x.reshape(-1, H, 64)
    lo = o.rb(t(p["hid"]) @ t(p["w2"]))
    w_raw = o.rb(lo + t(p["td"]))
    decay = hd(o.exp(-o.exp(w_raw)))
    r, k, v, u, S = hd(t(p["r"])), hd(t(p["k"])), hd(t(p["v"])), hd(t(p["u"])), t(p["S"])
    kv = k[..., :, None] * v[..., None, :]                                       # [key i][value j]
    y = o.rb(((u[..., :, None] * kv + S) * r[..., :, None]).sum(-2))
    S = S * decay[..., :, None] + kv
    dlt = y - y.mean(-1, keepdim=True)
    gn = o.rb(dlt * o.rsqrt((dlt * dlt).mean(-1, keepdim=True) + EPS_GN) * hd(t(p["ln_w"])) + hd(t(p["ln_b"])))
    gg = hd(t(p["g"]))
    sg = o.rb(gg / (1 + o.exp(-gg)))
    return {"tmix6_out": (gn * sg).reshape(B, H * 64), "tmix6_state": S, "w_raw": hd(w_raw)}


def floors(name, p):
    """The fp32 evaluations of the staged reference against the fp64 one (VRWKV_TEST_NOTES=1, CPU inputs)."""
    if not NOTES:
        return
    want = head_ref(O64, p)
    for label, o in (("fp32", Ops(torch.float32)), ("fp32 nudged", Ops(torch.float32, True))):
        got = head_ref(o, p)
        print(f"[decode6] floor {name} {label}: tmix6_out rel-RMS {rel_rms(rb64(got['tmix6_out']), rb64(want['tmix6_out'])):.3e}  "
              f"tmix6_state rel-RMS {rel_rms(got['tmix6_state'], want['tmix6_state']):.3e}")


@pytest.mark.parametrize("backend,B,H,Dd", _params(HEAD_CASES))
def test_tmix6_head(backend, be, B, H, Dd):
    g = be.gen(1000 * B + 10 * H + Dd)
    p = head_inputs(be, g, B, H, Dd)
    C = H * 64
    p["td"][3], p["td"][C - 2] = 2.0, -30.0                                     # a decay of about exp(-7) and one of exactly 1
    tag = f"tmix6_head/B{B}H{H}-D{Dd}"
    res = run_head(be, p)
    same_bits(res, run_head(be, p))
    ref = head_ref(O64, p)
    chain(be, "tmix6_out", res["out"][:-1], ref["tmix6_out"], f"{tag} out")
    chain(be, "tmix6_state", res["state"][:-1].view(B, H, 64, 64), ref["tmix6_state"], f"{tag} state")
    group_bias(res["out"][:-1], ref["tmix6_out"], f"{tag} out")
    if be.name == "emu":
        floors(tag, p)


@pytest.mark.parametrize("backend,B,H,Dd", _params(HEAD_CASES))
def test_tmix6_head_decay_rows(backend, be, B, H, Dd):
    """Head (0, 0) with k = 0: S' = diag(decay) S exactly, so every key row shows its decay exp(-exp(bf16 w_raw)) to fp32 accuracy (two 1-ulp
    exponentials and one product: < 5e-7), asserted for each of the 64 rows at 2e-6.  The one legitimate way for a row to differ is a tie:
    the kernel sums lo in fp32 -- d_decay / 32 FMAs per thread, then 32 partial sums added in a row: at most d_decay / 32 + 32 roundings
    behind any term -- and where the fp64 lo lies closer to a bf16 rounding boundary than that sum's worst-case error,
    (d_decay / 32 + 32) 2^-24 sum |hid w2|, either neighbour is a correct rounding (a few % of rows: boundaries are dense where lo is small).
    So the inputs are drawn again from the same generator until the fp64 reference alone says that no row of the head is in that
    position; then no row is left out.  The addition bf16(lo) + time_decay leaves no such freedom: the sum of two bf16 values is exact
    in fp32 (and where lo is too small for that, the sum is nowhere near a boundary), so kernel and reference round the same number,
    an exact midpoint included."""
    g = be.gen(2000 * B + 10 * H + Dd)
    for draw in range(200):
        p = head_inputs(be, g, B, H, Dd)
        hid, w2 = p["hid"][0].double(), p["w2"][:, :64].double()
        lo, slack = hid @ w2, (hid.abs() @ w2.abs()) * (Dd // 32 + 32) * 2.0 ** -24
        if not bool((rb64(lo - slack) != rb64(lo + slack)).any()):
            break
    else:
        raise AssertionError("no draw without a tied row")
    p["k"].view(B, H, 64)[0, 0] = 0
    res = run_head(be, p)
    ref = head_ref(O64, p)
    S0, S1 = p["S"][0, 0].double(), res["state"][0].double()
    decay = torch.exp(-torch.exp(ref["w_raw"][0, 0]))                           # per key row i
    err = ((S1 - S0 * decay[:, None]).abs() / (S0 * decay[:, None]).abs().clamp_min(1e-30)).amax(dim=1)
    if NOTES:
        print(f"[decode6] {be.name} tmix6_head/B{B}H{H}-D{Dd} decay rows: worst {float(err.max()):.3e} (row {int(err.argmax())}), draw {draw}")
    assert float(err.max()) < 2e-6, f"decay of head (0, 0): key row {int(err.argmax())} off by {float(err.max()):.3e}"
    chain(be, "tmix6_out", res["out"][:-1], ref["tmix6_out"], "decay rows out")


@pytest.mark.parametrize("backend,B,H,Dd", _params(HEAD_CASES))
def test_tmix6_head_zero_state_is_the_bonus(backend, be, B, H, Dd):
    """The last head from a zero state: y is the bonus term v[j] sum_i r[i] u[i] k[i] alone and the new state is the outer product k v^T,
    exact in fp32 (products of two bf16 values)."""
    g = be.gen(3000 * B + 10 * H + Dd)
    p = head_inputs(be, g, B, H, Dd)
    p["S"][B - 1, H - 1] = 0
    res = run_head(be, p)
    hd = lambda x: x.view(B, H, 64)[B - 1, H - 1].double()
    r, k, v, u = hd(p["r"]), hd(p["k"]), hd(p["v"]), p["u"].view(H, 64)[H - 1].double()
    assert torch.equal(res["state"][B * H - 1].double(), k[:, None] * v[None, :]), "zero state: S' = k v^T"
    y = rb64(v * (r * u * k).sum())
    dlt = y - y.mean()
    gn = rb64(dlt * torch.rsqrt((dlt * dlt).mean() + EPS_GN) * p["ln_w"].view(H, 64)[H - 1].double() + p["ln_b"].view(H, 64)[H - 1].double())
    gg = hd(p["g"])
    want = gn * rb64(gg * torch.sigmoid(gg))
    chain(be, "tmix6_out", res["out"][B - 1, (H - 1) * 64:], want, "zero state out")


# ------------------------------------------------------------------------------------------------ gated GEMV
GATED_ARGT = [I, I] + [VP] * 10 + [L]


def gated_jobs(be, g, B, K, Ns, ones=False):
    jobs = []
    for i, N in enumerate(Ns):
        gate = torch.ones(B, N, dtype=torch.bfloat16, device=be.dev) if ones else torch.sigmoid(torch.randn(B, N, generator=g, device=be.dev)).bfloat16()
        jobs.append(dict(W=rnd(be, g, N, K, scale=K ** -0.5), x=rnd(be, g, B, K), act=i % 4, res=rnd(be, g, B, N) if i % 2 == 0 else None, gate=gate))
    return jobs


def run_gated(be, B, jobs, copy=None):
    ys = [nan_rows(be, B, j["W"].shape[0]) for j in jobs]
    src, dst, elems = copy if copy is not None else (None, None, 0)
    be.call("vrwkv_gemv_gated_copy_bf16", GATED_ARGT, len(jobs), B, arr([j["W"] for j in jobs]), arr([j["x"] for j in jobs]),
            arr([j["res"] for j in jobs]), arr([j["gate"] for j in jobs]), arr(ys), ints([j["W"].shape[0] for j in jobs]),
            ints([j["W"].shape[1] for j in jobs]), ints([j["act"] for j in jobs]), P(src), P(dst), elems)
    written({f"y{j}": y for j, y in enumerate(ys)}, None, 0)
    return ys


@pytest.mark.parametrize("backend,path,B", _params([(p, B) for p, _, _ in GATED for B in (1, 4)]))
def test_gemv_gated(backend, be, path, B):
    """Every N of the path as the jobs of one launch (ragged against the path's rows per workgroup), every activation, with and without
    a residual, with the copy side job; with gate = 1 and no copy the plain entry's bits."""
    _, K, Ns = next(c for c in GATED if c[0] == path)
    g = be.gen(K + B)
    jobs = gated_jobs(be, g, B, K, Ns)
    src, dst = rnd(be, g, B * 64 + 8), torch.full((B * 64 + 8,), float("nan"), dtype=torch.bfloat16, device=be.dev)
    ys = run_gated(be, B, jobs, copy=(src, dst, B * 64))
    same_bits(dict(enumerate(ys)), dict(enumerate(run_gated(be, B, jobs))))
    assert torch.equal(bits(dst[:B * 64]), bits(src[:B * 64])) and bool(torch.isnan(dst[B * 64:].float()).all()), "copy side job"
    act64 = lambda v, a: [v, torch.tanh(v), torch.sigmoid(v), torch.relu(v) ** 2][a]
    got, want = [], []
    for j, y in zip(jobs, ys):
        ref = j["gate"].double() * act64(j["x"].double() @ j["W"].double().t(), j["act"])
        want.append((ref + j["res"].double() if j["res"] is not None else ref).reshape(-1))
        got.append(y[:-1].reshape(-1))
    CHECKS.act(be, torch.cat(got), torch.cat(want), f"gated/{path}/B{B}", guard=False)
    group_bias(torch.cat(got), torch.cat(want), f"gated/{path}/B{B}")
    ones = gated_jobs(be, g, B, K, Ns, ones=True)
    plain = [nan_rows(be, B, j["W"].shape[0]) for j in ones]
    be.call("vrwkv_gemv_multi_bf16", [I, I] + [VP] * 7, len(ones), B, arr([j["W"] for j in ones]), arr([j["x"] for j in ones]),
            arr([j["res"] for j in ones]), arr(plain), ints([j["W"].shape[0] for j in ones]), ints([j["W"].shape[1] for j in ones]),
            ints([j["act"] for j in ones]))
    same_bits(dict(enumerate(run_gated(be, B, ones))), dict(enumerate(plain)))


# ------------------------------------------------------------------------------------------------ argument rejections
def _nan_like(be, *shape, dtype=torch.bfloat16):
    return torch.full(shape, float("nan"), dtype=dtype, device=be.dev)


def _untouched(*bufs):
    for b in bufs:
        assert bool(torch.isnan(b.float()).all()), "a rejected call wrote to an output"


# The refusal tables are read off the entries as they stand: every count at 0 and one past its cap, every width just off its modulus,
# every pointer NULL in turn and 2 bytes (fp32: 4) off a 16-byte boundary; the gated GEMV alone has pointers it does not check (gate,
# res, y: element accesses), shown by an accepted call.  "Two faults" expect the code of the check that comes first.
# every buffer holds 5 batch rows: no case depends on being refused to stay in bounds
@pytest.mark.parametrize("backend", _params([()]))
def test_rejects_step(backend, be):
    g = be.gen(61)
    B, H = 2, 2
    names = ("r", "k", "v", "w", "u", "state", "y")
    t = {n: rnd(be, g, 5 * H * 64 + 8) for n in names[:5]}
    t["y"], t["state"] = _nan_like(be, 5 * H * 64 + 8), _nan_like(be, 5 * H * 4096 + 4, dtype=torch.float32)
    y, state = t["y"], t["state"]

    def go(B=B, H=H, null=(), off=()):
        ad = [VP(0 if n in null else t[n].data_ptr() + ((4 if n == "state" else 2) if n in off else 0)) for n in names]
        return rc_of(be, "vrwkv_wkv6_step_bf16", STEP_ARGT, B, H, *ad)

    assert go(B=0) == EINVAL and go(B=5) == EINVAL and go(H=0) == EINVAL
    assert go(H=129) == ESHAPE                                                  # C = 8256
    for name in names:
        assert go(null=(name,)) == EINVAL, name
        assert go(off=(name,)) == EALIGN, name
    # two faults
    assert go(B=5, H=129) == EINVAL and go(H=129, null=("r",)) == EINVAL and go(H=129, off=("r",)) == ESHAPE
    _untouched(y, state)
    state.zero_()
    assert go() == 0
    assert bool(torch.isfinite(y[:B * H * 64].float()).all()) and bool(torch.isnan(y[B * H * 64:].float()).all())


@pytest.mark.parametrize("backend", _params([()]))
def test_rejects_ddlerp(backend, be):
    g = be.gen(62)
    B, C, D = 2, 128, 32
    h, hid, w2 = rnd(be, g, 5 * C + 8), rnd(be, g, 5 * 5 * 64 + 8), rnd(be, g, 5 * 64 * C + 8)
    prev = rnd(be, g, 5 * C + 8)
    keep = prev.clone()
    maa = [rnd(be, g, C + 8) for _ in range(5)]
    outs = [_nan_like(be, 5 * C + 8) for _ in range(5)]

    def go(B=B, C=C, D=D, h=h.data_ptr(), prev=prev.data_ptr(), maa=maa, outs=outs, w2=w2.data_ptr(), hid=hid.data_ptr()):
        return rc_of(be, "vrwkv_decode6_ddlerp_bf16", DD_ARGT, B, C, D, VP(h), VP(prev), VP(hid), VP(w2), arr(maa) if maa is not None else None,
                     arr(outs) if outs is not None else None)

    assert go(B=0) == EINVAL and go(B=5) == EINVAL
    assert go(C=72) == ESHAPE and go(C=0) == ESHAPE and go(C=8256) == ESHAPE
    assert go(D=48) == ESHAPE and go(D=0) == ESHAPE and go(D=128) == ESHAPE
    assert go(h=None) == EINVAL and go(prev=None) == EINVAL and go(maa=None) == EINVAL and go(outs=None) == EINVAL
    assert go(hid=None) == EINVAL and go(w2=None) == EINVAL
    assert go(maa=maa[:2] + [None] + maa[3:]) == EINVAL and go(outs=outs[:4] + [None]) == EINVAL
    assert go(h=h.data_ptr() + 2) == EALIGN and go(prev=prev.data_ptr() + 2) == EALIGN and go(w2=w2.data_ptr() + 2) == EALIGN
    assert go(hid=hid.data_ptr() + 2) == EALIGN
    assert go(outs=outs[:3] + [outs[3].data_ptr() + 2] + outs[4:]) == EALIGN and go(maa=[maa[0].data_ptr() + 2] + maa[1:]) == EALIGN
    # two faults
    assert go(B=5, C=72) == EINVAL and go(C=72, h=h.data_ptr() + 2) == ESHAPE and go(h=None, D=48) == EINVAL
    assert go(maa=maa[:2] + [None] + maa[3:], h=h.data_ptr() + 2) == EINVAL
    assert go(maa=[maa[0].data_ptr() + 2] + maa[1:], outs=outs[:4] + [None]) == EINVAL      # a NULL anywhere in the arrays before any alignment
    _untouched(*outs)
    assert torch.equal(bits(prev), bits(keep)), "a rejected call replaced the carried row"
    assert go() == 0
    assert torch.equal(bits(prev[:B * C]), bits(h[:B * C])) and torch.equal(bits(prev[B * C:]), bits(keep[B * C:]))


@pytest.mark.parametrize("backend", _params([()]))
def test_rejects_tmix6_head(backend, be):
    g = be.gen(63)
    B, H = 2, 2
    p = head_inputs(be, g, 5, H, 128)
    names = ("r", "k", "v", "g", "hid", "w2", "td", "u", "ln_w", "ln_b", "state", "out")
    t = {n: p[n] for n in names[:10]}
    t["out"], t["state"] = _nan_like(be, 5 * H * 64 + 8), _nan_like(be, 5 * H * 4096 + 4, dtype=torch.float32)
    out, state = t["out"], t["state"]

    def go(B=B, H=H, Dd=64, null=(), off=()):
        ad = [VP(0 if n in null else t[n].data_ptr() + ((4 if n == "state" else 2) if n in off else 0)) for n in names]
        return rc_of(be, "vrwkv_decode6_tmix_head_bf16", HEAD_ARGT, B, H, Dd, *ad[:10], EPS_GN, *ad[10:])

    assert go(B=0) == EINVAL and go(B=5) == EINVAL and go(H=0) == EINVAL
    assert go(Dd=96) == ESHAPE and go(Dd=32) == ESHAPE and go(Dd=256) == ESHAPE and go(Dd=0) == ESHAPE and go(H=129) == ESHAPE
    for name in names:
        assert go(null=(name,)) == EINVAL, name
        assert go(off=(name,)) == EALIGN, name
    # two faults
    assert go(B=5, Dd=96) == EINVAL and go(Dd=96, null=("w2",)) == EINVAL and go(Dd=96, off=("r",)) == ESHAPE and go(H=129, off=("state",)) == ESHAPE
    _untouched(out, state)


@pytest.mark.parametrize("backend", _params([()]))
def test_rejects_gemv_gated(backend, be):
    g = be.gen(64)
    B, N, K = 2, 9, 64
    W, x, gate, y, res = rnd(be, g, N + 1, K), rnd(be, g, 5 + 1, K), rnd(be, g, 5 + 1, N), _nan_like(be, 5 + 1, N), rnd(be, g, 5 + 1, N)
    src, dst = rnd(be, g, 64), _nan_like(be, 64)

    def go(n=1, B=B, W=W.data_ptr(), x=x.data_ptr(), y=y.data_ptr(), res=None, N=N, K=K, gate=[gate], null=(), s=None, d=None, elems=0):
        m = max(n, 1)
        a = dict(W=arr([W] * m), x=arr([x] * m), res=arr([res] * m) if res is not None else None, gate=arr(gate * m) if gate is not None else None,
                 y=arr([y] * m), N=ints([N] * m), K=ints([K] * m), act=ints([0] * m))
        return rc_of(be, "vrwkv_gemv_gated_copy_bf16", GATED_ARGT, n, B, *[None if k in null else a[k] for k in ("W", "x", "res", "gate", "y", "N", "K", "act")],
                     VP(s), VP(d), elems)

    sp, dp = src.data_ptr(), dst.data_ptr()
    assert go(n=0) == EINVAL and go(n=9) == EINVAL and go(B=0) == EINVAL and go(B=5) == EINVAL
    assert go(gate=None) == EINVAL and go(gate=[None]) == EINVAL
    for name in ("W", "x", "y", "N", "K", "act"):
        assert go(null=(name,)) == EINVAL, name
    assert go(W=None) == ESHAPE and go(x=None) == ESHAPE and go(y=None) == ESHAPE
    assert go(K=60) == ESHAPE and go(K=0) == ESHAPE and go(N=0) == ESHAPE
    assert go(W=W.data_ptr() + 2) == EALIGN and go(x=x.data_ptr() + 2) == EALIGN
    assert go(s=sp, d=dp, elems=12) == ESHAPE and go(s=sp, d=dp, elems=-8) == EINVAL
    assert go(s=None, d=dp, elems=8) == EINVAL and go(s=sp, d=None, elems=8) == EINVAL
    assert go(s=sp, d=dp + 2, elems=8) == EALIGN and go(s=sp + 2, d=dp, elems=8) == EALIGN
    # two faults: the gate array first, then the launcher's order (counts, copy side job, job by job: shape, alignment, gate)
    assert go(gate=None, n=0) == EINVAL and go(gate=[None], K=60) == ESHAPE and go(gate=[None], W=W.data_ptr() + 2) == EALIGN
    assert go(s=sp, d=dp, elems=12, gate=[None]) == ESHAPE and go(B=5, K=60) == EINVAL
    _untouched(y, dst)
    y2 = _nan_like(be, 5 + 1, N)
    assert go(y=y2.data_ptr() + 2, res=res.data_ptr() + 2, gate=[gate.data_ptr() + 2]) == 0        # gate, res and y: element accesses, not checked
    assert bool(torch.isfinite(y2.reshape(-1)[1:1 + B * N].float()).all()) and bool(torch.isnan(y2.reshape(-1)[1 + B * N:].float()).all())
    _untouched(y, dst)
    assert go() == 0
    assert bool(torch.isfinite(y[:B].float()).all()) and bool(torch.isnan(y[B:].float()).all())
