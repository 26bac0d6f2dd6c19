"""The element-wise glue of the time-mix (csrc/tmix_fused.hip: mix, ddmix, decay, kva, post, gn_silu and the colsum that finishes
their parameter gradients) at the shapes where its backward kernels change their code path, through the C ABI, on two backends with
the same test bodies: the host lockstep emulator (CPU tensors, no marker) and the product library (CUDA tensors, `gpu` marker).

What picks the path (see SHAPES): the grid caps -- bwd_grid = min(ceil(ntok / 16), 1024) workgroups with contiguous token ranges, 768
strided workgroups for kva_bwd / post_bwd with C / 8 <= 256 --, the second trip of colsum's row loop (more than 64 partial rows), the
row width (kva_bwd / post_bwd <256> prefetching, <512>, <1024>; C / 8 threads, a partial wave for C = 192 and C = 2112) and the
channel loop of mix_bwd (C > 2048).

Reference: torch autograd in fp64 on the same bf16 inputs (ref_mix, ref_decay, ref_kva, ref_post, ref_gn_silu below), evaluated on
the backend's device.  The group norm of ref_post / ref_gn_silu is spelled out in elementary ops (group_norm64) instead of
F.group_norm: torch 2.10 for ROCm 7.0 returns wrong fp64 weight and bias gradients from F.group_norm on the MI355X for more than 128
rows (at 129 x 64, 1125 x 64 and 1125 x 256 every odd channel of the weight gradient comes out at exactly twice the CPU's value, the
even ones unrelated to it; 128 x 64 and 37 x 2048 agree to 4e-16), while group_norm64 agrees with the CPU to 3e-15 on both devices.
Every case asserts
  1. activations and activation gradients: tests.parity.bf16_close against the reference rounded once, tol 1e-3, flips <= FLIP;
  2. parameter gradients in fp32, before any bf16 conversion, per vector: max_c |got_c - ref_c| / rms_c(ref) <= PERR (a per-channel
     maximum: one dropped partial row or one wrong channel shows) and tests.parity.group_bias (a systematic factor);
  3. outputs, dparams and ws are NaN before the call (the partial rows that are sized but unused at the 768 cap included) and every
     buffer ends in a guard row: results finite everywhere, guards untouched;
  4. a second call is bit-identical (colsum sums in a fixed order);
  5. the forward kernels, by the same bf16_close.
Input edges ride along: decay with h + w0 at +-100 (the exponential under- and overflows: finite, the 0 / 1 limits of the reference),
post / gn_silu with an all-zero row of y and a head that is constant over its 64 channels (zero variance), mix / ddmix with
integer-valued x and mu = 1 (the shifted row bit-exactly, zeros at every sample start).

Bounds.  FLIP and PERR are 4 x the worst value observed over all cases of a backend (the arithmetic is deterministic; the margin is
for other seeds and other boxes), and have to stay at or below the project's 0.01 (FLIP_Y of test_wkv7_gpu.py) and 1e-4 (kva's
parameter gradients in test_emulated_tmix.py).  VRWKV_TEST_NOTES=1 prints every figure and the running worst.
Observed (worst case over the module, the case that gave it):
  emulator (host libm):  flips 9.191e-04 (kva ragged_pair vres+v dk: one element of 1088), parameter gradients 1.514e-06
                         (gn_silu lb1024_full dln_w)  ->  FLIP 3.7e-3, PERR 6.1e-6
  MI355X (hardware exp / log / rsqrt / rcp):  flips 9.191e-04 (kva ragged_pair vres+v+f dal and vres+k v2: one element of 1088),
                         parameter gradients 1.255e-06 (gn_silu lb1024_first dln_w)  ->  FLIP 3.7e-3, PERR 5.1e-6
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests.shape_checks import Checks

L, I, F32, VP = ctypes.c_long, ctypes.c_int, ctypes.c_float, ctypes.c_void_p
EPS = 64e-5
TOL = 1e-3
FLIP = {"emu": 3.7e-3, "hip": 3.7e-3}         # 4 x observed (module docstring)
PERR = {"emu": 6.1e-6, "hip": 5.1e-6}

BACKENDS = ["emu", pytest.param("hip", marks=pytest.mark.gpu)]      # host lockstep emulator | product library on the MI355X
#   id                (B, T) of mix / ddmix;  ntok = B T for the rest          C     what it reaches
SHAPES = [
    ("one_token",       1, 1,    64),     # G = 1, nothing to prefetch
    ("ragged_pair",     1, 17,   64),     # G = 2, ranges of 8 and 9 tokens
    ("colsum_trip2",    3, 375,  64),     # G = 71: the second trip of colsum's row loop, 7 of its 64 row groups busy
    ("prefetch_cap",    3, 4115, 64),     # kva / post: G = 768 of 772 sized partial rows, 16-17 strided tokens each; the others 772
    ("range_cap",       3, 5471, 64),     # G = 1024 of 1026, contiguous ranges of 16-17 tokens
    ("partial_wave",    1, 37,   192),    # 24-thread workgroups, mix_bwd with 48
    ("pf_widest",       1, 37,   2048),   # <256> full
    ("nopf_first",      1, 37,   2112),   # <512> with 264 threads; mix_bwd's channel loop with a 16-thread second trip
    ("lb512_full",      1, 37,   4096),
    ("lb1024_first",    1, 37,   4160),
    ("lb1024_full",     1, 37,   8192),   # the largest C ok_c admits
    ("x_nopf_capped",   3, 4115, 2112),   # GPU only: the non-prefetching kernel beyond 768 workgroups (G = 772)
    ("x_pf_waves",      3, 5471, 256),    # GPU only: the prefetch cap with more than one wave per workgroup
]
FULL_MATRIX = ("ragged_pair", "nopf_first")
GPU_ONLY = ("x_nopf_capped", "x_pf_waves")
EMU_WIDE_T = 19                            # the emulator walks the wide rows (C >= 2048) with 19 tokens instead of 37


def _cases(configs_full=None, configs_rest=None):
    """(backend, shape[, config]) of one test: the full option matrix at FULL_MATRIX, `configs_rest` elsewhere; the GPU_ONLY shapes
    are not generated for the emulator."""
    out = []
    for b in BACKENDS:
        name, marks = (b, ()) if isinstance(b, str) else (b.values[0], b.marks)
        for sid, _, _, _ in SHAPES:
            if name == "emu" and sid in GPU_ONLY:
                continue
            for cfg in ([None] if configs_full is None else configs_full if sid in FULL_MATRIX else configs_rest):
                vals = (name, sid) if cfg is None else (name, sid, cfg)
                out.append(pytest.param(*vals, id="-".join(vals), marks=marks))
    return out


class Backend:
    def __init__(self, request, name):
        self.name = name
        if name == "hip":
            self.lib = request.getfixturevalue("hip_lib")
            assert torch.cuda.is_available(), "these cases need an MI355X"
            self.dev = torch.device("cuda:0")
            self.stream = VP(torch.cuda.current_stream(self.dev).cuda_stream)
        else:
            self.lib = request.getfixturevalue("emu_lib")
            self.dev = torch.device("cpu")
            self.stream = None

    def shape(self, sid):
        _, B, T, C = next(s for s in SHAPES if s[0] == sid)
        if self.name == "emu" and C >= 2048:
            T = EMU_WIDE_T
        return B, T, C

    def gen(self, seed):
        return torch.Generator(device=self.dev).manual_seed(seed)

    def rc(self, fn, argtypes, *args):
        f = getattr(self.lib, fn)
        f.argtypes, f.restype = argtypes + [VP], I
        return f(*args, self.stream)

    def call(self, fn, argtypes, *args):
        rc = self.rc(fn, argtypes, *args)
        assert rc == 0, (fn, rc)

    def ws_floats(self, ntok, C, nvec):
        f = self.lib.vrwkv_param_grad_ws_floats
        f.argtypes, f.restype = [L, I, I], L
        return int(f(ntok, C, nvec))


@pytest.fixture
def be(request, backend):
    return Backend(request, backend)


def P(t):
    return VP(t.data_ptr()) if t is not None else None


def PA(ts):
    return (VP * len(ts))(*[t.data_ptr() for t in ts])


def rnd(be, g, *shape, scale=1.0, shift=0.0):
    return (torch.randn(*shape, generator=g, device=be.dev) * scale + shift).bfloat16()


def unif(be, g, *shape):
    return torch.rand(*shape, generator=g, device=be.dev).bfloat16()


def f64(ts, grad=True):
    return [t.double().requires_grad_(grad) for t in ts]


# ------------------------------------------------------------------------------------------------ references (any float dtype)
def ref_mix(x, mus, mm=None):
    """x (B, T, C); out_j = x + (x[t-1] - x) (mu_j [+ mm_j]), zeros before every sample's first token."""
    xx = F.pad(x, (0, 0, 1, -1)) - x
    return tuple(x + xx * (m if mm is None else m + mm[j]) for j, m in enumerate(mus))


def ref_decay(h, w0):
    return -F.softplus(-(w0 + h)) - 0.5


def ref_kva(k, v, vf, vl, al, k_k, k_a, a0, v0, has_vres=True):
    """(ntok, C) rows, heads of 64 channels; returns (k2, v2, z, b), v2 = None without the value residual."""
    ntok, C = k.shape
    a = torch.sigmoid(a0 + al)
    v2 = v + (vf - v) * torch.sigmoid(v0 + vl) if has_vres else None
    kk = F.normalize((k * k_k).view(ntok, C // 64, 64), dim=-1, p=2.0).view(ntok, C)
    k2 = k * (1 + (a - 1) * k_a)
    return k2, v2, -kk, kk * a


def group_norm64(y, ln_w, ln_b, eps=EPS):
    """F.group_norm(y, C // 64, ln_w, ln_b, eps) of (ntok, C) rows, spelled out (biased variance) so that autograd differentiates
    elementary ops on every device instead of calling the library's fused group-norm backward."""
    ntok, C = y.shape
    yh = y.view(ntok, C // 64, 64)
    mean = yh.mean(dim=-1, keepdim=True)
    var = (yh - mean).pow(2).mean(dim=-1, keepdim=True)
    return ((yh - mean) * torch.rsqrt(var + eps)).view(ntok, C) * ln_w + ln_b


def ref_post(y, r, k, v, g, ln_w, ln_b, r_k, eps=EPS):
    ntok, C = y.shape
    H = C // 64
    x = group_norm64(y, ln_w, ln_b, eps)
    bonus = (r.view(ntok, H, 64) * k.view(ntok, H, 64) * r_k.view(H, 64)).sum(dim=-1, keepdim=True) * v.view(ntok, H, 64)
    return (x + bonus.view(ntok, C)) * g


def ref_gn_silu(y, gg, ln_w, ln_b, eps=EPS):
    return group_norm64(y, ln_w, ln_b, eps) * F.silu(gg)


# ------------------------------------------------------------------------------------------------ buffers and checks
def nan_rows(be, rows, C, dtype=torch.bfloat16):
    """`rows` rows to be written plus one guard row, all NaN."""
    return torch.full((rows + 1, C), float("nan"), dtype=dtype, device=be.dev)


def nan_ws(be, ntok, C, nvec):
    return torch.full((be.ws_floats(ntok, C, nvec) + C,), float("nan"), dtype=torch.float32, device=be.dev)


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def written(res, ws, ws_used):
    """Every result finite up to its guard row, the guards (and the C floats after ws) still NaN.  The rows inside ws are not looked
    at: that a NaN partial row which the capped grid leaves unwritten (768 .. 771 at the prefetch cap) is never summed shows only
    through dparams being finite."""
    for name, buf in res.items():
        assert bool(torch.isfinite(buf[:-1].float()).all()), f"{name}: not finite (unwritten or overflowed)"
        assert bool(torch.isnan(buf[-1].float()).all()), f"{name}: guard row written"
    if ws is not None:
        assert bool(torch.isnan(ws[ws_used:]).all()), "ws: written past vrwkv_param_grad_ws_floats"


def same_bits(a, b):
    for name in a:
        assert torch.equal(bits(a[name]), bits(b[name])), f"{name}: the second call differs"


CHECKS = Checks("glue", FLIP, PERR, TOL)
note, act, par = CHECKS.note, CHECKS.act, CHECKS.par


def _mix_case(be, sid, M, dup3, dd):
    B, T, C = be.shape(sid)
    ntok = B * T
    g = be.gen(1000 * M + 7 * ntok + C + dup3)
    x = rnd(be, g, ntok, C)
    mus = [unif(be, g, C) for _ in range(M)]
    mm = [rnd(be, g, ntok, C, scale=0.2) for _ in range(M)] if dd else None
    douts = [rnd(be, g, ntok, C) for _ in range(M)]
    d3b = rnd(be, g, ntok, C) if dup3 else None
    tag = f"{'ddmix' if dd else 'mix'}/{sid}/M{M}{'+dup3' if dup3 else ''}"

    def fwd(xin, muin, mmin):
        outs = [nan_rows(be, ntok, C) for _ in range(M)]
        if dd:
            be.call("vrwkv_ddmix_fwd_bf16", [L, I, I] + [VP] * 4, ntok, T, C, P(xin), PA(muin), PA(mmin), PA(outs))
        else:
            be.call("vrwkv_mix_fwd_bf16", [L, I, I, I] + [VP] * 3, ntok, T, C, M, P(xin), PA(muin), PA(outs))
        return {f"out{j}": o for j, o in enumerate(outs)}

    def bwd():
        dx, dmu, ws = nan_rows(be, ntok, C), nan_rows(be, M, C, torch.float32), nan_ws(be, ntok, C, M)
        res = {"dx": dx, "dmu": dmu}
        if dd:
            dmm = [nan_rows(be, ntok, C) for _ in range(M)]
            res.update({f"dmm{j}": o for j, o in enumerate(dmm)})
            be.call("vrwkv_ddmix_bwd_bf16", [L, I, I] + [VP] * 8, ntok, T, C, P(x), PA(mus), PA(mm), PA(douts), P(dx), PA(dmm), P(dmu), P(ws))
        else:
            be.call("vrwkv_mix_bwd2_bf16", [L, I, I, I] + [VP] * 7, ntok, T, C, M, P(x), PA(mus), PA(douts), P(d3b), P(dx), P(dmu), P(ws))
        written(res, ws, be.ws_floats(ntok, C, M))
        return res

    o1, o2 = fwd(x, mus, mm), fwd(x, mus, mm)
    written(o1, None, 0)
    same_bits(o1, o2)
    r1, r2 = bwd(), bwd()
    same_bits(r1, r2)

    xd, = f64([x.view(B, T, C)])
    md = f64(mus)
    mmd = f64([t.view(B, T, C) for t in mm]) if dd else None
    ref = ref_mix(xd, md, mmd)
    gr = [d.double().view(B, T, C) for d in douts]
    if dup3:
        gr[3] = gr[3] + d3b.double().view(B, T, C)
    torch.autograd.backward(ref, gr)
    for j in range(M):
        act(be, o1[f"out{j}"], ref[j], f"{tag} out{j}")
        par(be, r1["dmu"][j], md[j].grad, f"{tag} dmu{j}")
        if dd:
            act(be, r1[f"dmm{j}"], mmd[j].grad, f"{tag} dmm{j}")
    act(be, r1["dx"], xd.grad, f"{tag} dx")

    # exact shift indexing: integer-valued x (all fp32 arithmetic exact) and lerp weight 1 give exactly the previous token, and exactly
    # zero at the first token of every sample
    xi = torch.randint(-8, 9, (ntok, C), generator=g, device=be.dev).bfloat16()
    ones = [torch.ones(C, dtype=torch.bfloat16, device=be.dev) for _ in range(M)]
    zeros = [torch.zeros(ntok, C, dtype=torch.bfloat16, device=be.dev) for _ in range(M)] if dd else None
    for name, o in fwd(xi, ones, zeros).items():
        o, xv = o[:-1].view(B, T, C), xi.view(B, T, C)
        assert torch.equal(o[:, 1:], xv[:, :-1]) and not bool(o[:, 0].any()), f"{tag} {name}: shifted rows"


MIX_ALL = ["M1", "M2", "M6", "M6+dup3"]


@pytest.mark.parametrize("backend,sid,cfg", _cases(MIX_ALL, ["M6+dup3"]))
def test_mix(backend, be, sid, cfg):
    _mix_case(be, sid, int(cfg[1]), cfg.endswith("dup3"), dd=False)


@pytest.mark.parametrize("backend,sid", _cases())
def test_ddmix(backend, be, sid):
    _mix_case(be, sid, 5, False, dd=True)


# ------------------------------------------------------------------------------------------------ decay
@pytest.mark.parametrize("backend,sid", _cases())
def test_decay(backend, be, sid):
    B, T, C = be.shape(sid)
    ntok = B * T
    g = be.gen(3 * ntok + C)
    h, w0, dw = rnd(be, g, ntok, C, scale=3.0), rnd(be, g, C, scale=2.0), rnd(be, g, ntok, C)
    # h + w0 at about +-100: exp(-|u|) underflows in the forward, exp(u) overflows in the backward's sigmoid
    for n, c, val in ((0, 3, 100.0), (ntok - 1, 5, -100.0), (ntok // 2, C - 1, 100.0), (ntok // 2, 0, -100.0)):
        h[n, c] = val
    tag = f"decay/{sid}"

    def run():
        w, dh, dw0, ws = nan_rows(be, ntok, C), nan_rows(be, ntok, C), nan_rows(be, 1, C, torch.float32), nan_ws(be, ntok, C, 1)
        be.call("vrwkv_decay_fwd_bf16", [L, I] + [VP] * 3, ntok, C, P(h), P(w0), P(w))
        be.call("vrwkv_decay_bwd_bf16", [L, I] + [VP] * 6, ntok, C, P(h), P(w0), P(dw), P(dh), P(dw0), P(ws))
        res = {"w": w, "dh": dh, "dw0": dw0}
        written(res, ws, be.ws_floats(ntok, C, 1))
        return res

    r1, r2 = run(), run()
    same_bits(r1, r2)
    hd, wd = f64([h, w0])
    ref = ref_decay(hd, wd)
    ref.backward(dw.double())
    act(be, r1["w"], ref, f"{tag} w")
    act(be, r1["dh"], hd.grad, f"{tag} dh")
    par(be, r1["dw0"][0], wd.grad, f"{tag} dw0")
    assert float(r1["w"][:-1].float().max()) <= -0.5
    # the limits themselves: u = +100 -> w = -0.5, dh = 0;  u = -100 -> w = u - 0.5 (softplus is the identity), dh = dw
    assert float(r1["w"][0, 3]) == -0.5 and float(r1["dh"][0, 3]) == 0.0
    assert float(r1["dh"][ntok - 1, 5]) == float(dw[ntok - 1, 5])


# ------------------------------------------------------------------------------------------------ kva
KVA_ALL = ["novres", "novres+k"] + ["vres" + "".join(s for s, on in zip(("+k", "+v", "+f"), (a, b, c)) if on)
                                    for a in (0, 1) for b in (0, 1) for c in (0, 1)]


@pytest.mark.parametrize("backend,sid,cfg", _cases(KVA_ALL, ["vres+k+v+f", "novres"]))
def test_kva(backend, be, sid, cfg):
    """cfg: has_vres, +k = dk2_second, +v = dv2_second, +f = dvfirst_in."""
    B, T, C = be.shape(sid)
    ntok = B * T
    vres = cfg.startswith("vres")
    g = be.gen(5 * ntok + C + 17 * KVA_ALL.index(cfg))
    k, v, vf, vl, al = [rnd(be, g, ntok, C) for _ in range(5)]
    k_k, k_a, a0, v0 = [rnd(be, g, C, scale=0.5) for _ in range(4)]
    dk2, dv2, dz, db = [rnd(be, g, ntok, C) for _ in range(4)]
    dk2b = rnd(be, g, ntok, C) if "+k" in cfg else None
    dv2b = rnd(be, g, ntok, C) if "+v" in cfg else None
    dvf_in = rnd(be, g, ntok, C) if "+f" in cfg else None
    tag = f"kva/{sid}/{cfg}"
    vin = (v, vf, vl) if vres else (None, None, None)

    def run():
        fw = {n: nan_rows(be, ntok, C) for n in (("k2", "v2", "z", "b") if vres else ("k2", "z", "b"))}
        be.call("vrwkv_kva_fwd_bf16", [L, I, I] + [VP] * 13, ntok, C, int(vres), P(k), *map(P, vin), P(al), P(k_k), P(k_a), P(a0),
                P(v0 if vres else None), P(fw["k2"]), P(fw.get("v2")), P(fw["z"]), P(fw["b"]))
        bw = {n: nan_rows(be, ntok, C) for n in (("dk", "dv", "dvfirst", "dvl", "dal") if vres else ("dk", "dal"))}
        pg, ws = nan_rows(be, 4, C, torch.float32), nan_ws(be, ntok, C, 4)
        be.call("vrwkv_kva_bwd3_bf16", [L, I, I] + [VP] * 23, ntok, C, int(vres), P(k), *map(P, vin), P(al), P(k_k), P(k_a), P(a0),
                P(v0 if vres else None), P(dk2), P(dv2 if vres else None), P(dz), P(db), P(dk2b), P(dv2b), P(dvf_in),
                P(bw["dk"]), P(bw.get("dv")), P(bw.get("dvfirst")), P(bw.get("dvl")), P(bw["dal"]), P(pg), P(ws))
        res = {**fw, **bw, "dparams": pg}
        written(res, ws, be.ws_floats(ntok, C, 4))
        return res

    r1, r2 = run(), run()
    same_bits(r1, r2)
    xs = f64([k, v, vf, vl, al, k_k, k_a, a0, v0])
    k2r, v2r, zr, br = ref_kva(*xs, has_vres=vres)
    gk2 = dk2.double() + (dk2b.double() if dk2b is not None else 0)
    outs, gs = [k2r, zr, br], [gk2, dz.double(), db.double()]
    if vres:
        outs.append(v2r)
        gs.append(dv2.double() + (dv2b.double() if dv2b is not None else 0))
    torch.autograd.backward(outs, gs)
    for name, r in (("k2", k2r), ("z", zr), ("b", br)) + ((("v2", v2r),) if vres else ()):
        act(be, r1[name], r, f"{tag} {name}")
    act(be, r1["dk"], xs[0].grad, f"{tag} dk")
    act(be, r1["dal"], xs[4].grad, f"{tag} dal")
    if vres:
        act(be, r1["dv"], xs[1].grad, f"{tag} dv")
        act(be, r1["dvfirst"], xs[2].grad + (dvf_in.double() if dvf_in is not None else 0), f"{tag} dvfirst")
        act(be, r1["dvl"], xs[3].grad, f"{tag} dvl")
    for j, name in enumerate(("dk_k", "dk_a", "da0", "dv0")):
        ref = xs[5 + j].grad
        par(be, r1["dparams"][j], ref if ref is not None else torch.zeros(C, dtype=torch.float64), f"{tag} {name}")


# ------------------------------------------------------------------------------------------------ post / gn_silu
def _gn_edges(y, ntok):
    """One all-zero row and one head that is constant over its 64 channels: zero variance, rstd = 1 / sqrt(eps)."""
    if ntok >= 2:
        y[ntok // 2] = 0.0
        y[ntok - 1, :64] = 1.5


@pytest.mark.parametrize("backend,sid", _cases())
def test_post(backend, be, sid):
    B, T, C = be.shape(sid)
    ntok = B * T
    g = be.gen(11 * ntok + C)
    y, r, k, v, gt = [rnd(be, g, ntok, C) for _ in range(5)]
    _gn_edges(y, ntok)
    ln_w, ln_b, r_k = rnd(be, g, C, scale=0.5, shift=1.0), rnd(be, g, C, scale=0.1), rnd(be, g, C, scale=0.3)
    dout = rnd(be, g, ntok, C)
    tag = f"post/{sid}"

    def run():
        res = {n: nan_rows(be, ntok, C) for n in ("out", "dy", "dr", "dk", "dv", "dg")}
        pg, ws = nan_rows(be, 3, C, torch.float32), nan_ws(be, ntok, C, 3)
        be.call("vrwkv_post_fwd_bf16", [L, I, F32] + [VP] * 9, ntok, C, EPS, P(y), P(r), P(k), P(v), P(gt), P(ln_w), P(ln_b), P(r_k), P(res["out"]))
        be.call("vrwkv_post_bwd_bf16", [L, I, F32] + [VP] * 16, ntok, C, EPS, P(y), P(r), P(k), P(v), P(gt), P(ln_w), P(ln_b), P(r_k), P(dout),
                P(res["dy"]), P(res["dr"]), P(res["dk"]), P(res["dv"]), P(res["dg"]), P(pg), P(ws))
        res["dparams"] = pg
        written(res, ws, be.ws_floats(ntok, C, 3))
        return res

    r1, r2 = run(), run()
    same_bits(r1, r2)
    xs = f64([y, r, k, v, gt, ln_w, ln_b, r_k])
    ref = ref_post(*xs)
    ref.backward(dout.double())
    act(be, r1["out"], ref, f"{tag} out")
    for name, x in zip(("dy", "dr", "dk", "dv", "dg"), xs):
        act(be, r1[name], x.grad, f"{tag} {name}")
    for j, name in enumerate(("dln_w", "dln_b", "dr_k")):
        par(be, r1["dparams"][j], xs[5 + j].grad, f"{tag} {name}")


@pytest.mark.parametrize("backend,sid", _cases())
def test_gn_silu(backend, be, sid):
    B, T, C = be.shape(sid)
    ntok = B * T
    g = be.gen(13 * ntok + C)
    y, gg, dout = [rnd(be, g, ntok, C) for _ in range(3)]
    _gn_edges(y, ntok)
    ln_w, ln_b = rnd(be, g, C, scale=0.2, shift=1.0), rnd(be, g, C, scale=0.2)
    tag = f"gn_silu/{sid}"

    def run():
        res = {n: nan_rows(be, ntok, C) for n in ("out", "dy", "dgg")}
        pg, ws = nan_rows(be, 2, C, torch.float32), nan_ws(be, ntok, C, 2)
        be.call("vrwkv_gn_silu_fwd_bf16", [L, I, F32] + [VP] * 5, ntok, C, EPS, P(y), P(gg), P(ln_w), P(ln_b), P(res["out"]))
        be.call("vrwkv_gn_silu_bwd_bf16", [L, I, F32] + [VP] * 9, ntok, C, EPS, P(y), P(gg), P(ln_w), P(ln_b), P(dout),
                P(res["dy"]), P(res["dgg"]), P(pg), P(ws))
        res["dparams"] = pg
        written(res, ws, be.ws_floats(ntok, C, 2))
        return res

    r1, r2 = run(), run()
    same_bits(r1, r2)
    xs = f64([y, gg, ln_w, ln_b])
    ref = ref_gn_silu(*xs)
    ref.backward(dout.double())
    act(be, r1["out"], ref, f"{tag} out")
    act(be, r1["dy"], xs[0].grad, f"{tag} dy")
    act(be, r1["dgg"], xs[1].grad, f"{tag} dgg")
    for j, name in enumerate(("dln_w", "dln_b")):
        par(be, r1["dparams"][j], xs[2 + j].grad, f"{tag} {name}")


# ------------------------------------------------------------------------------------------------ refusals, forwarding entries
EINVAL, ESHAPE = -1, -2                                   # VRWKV_EINVAL, VRWKV_ESHAPE of include/visualrwkv_hip.h
# Every vrwkv_* entry of tmix_fused.hip that returns a code (vrwkv_param_grad_ws_floats returns a size), its arguments in order:
# ntok T C M has eps n are the scalars; a name is a required pointer, name? an optional one (NULL in the valid call), name* one that
# has_vres requires, name[] an array of pointers (M of them, 5 for ddmix); > marks what the entry writes.
GLUE_ENTRIES = {
    "vrwkv_mix_fwd_bf16": "ntok T C M x mu[] >out[]",
    "vrwkv_mix_fwd_prev_bf16": "ntok T C M x x_prev? mu[] >out[]",
    "vrwkv_mix_bwd_bf16": "ntok T C M x mu[] dout[] >dx >dmu >ws",
    "vrwkv_mix_bwd2_bf16": "ntok T C M x mu[] dout[] dout3_second? >dx >dmu >ws",
    "vrwkv_mix_bwd_ln_bf16": "ntok T C M xn mean rstd ln_w ln_b mu[] dout[] dout3_second? >dx >dmu >ws",
    "vrwkv_mix_bwd_ln_packed_bf16": "ntok T C M xn mean rstd ln_w ln_b mu[] dout[] dout3_second? first? >dx >dmu >ws",
    "vrwkv_mix_bwd_ln_carry_bf16": "ntok T C M xn mean rstd ln_w ln_b mu[] dout[] dout3_second? y_prev? dy_last? >dy_prev? >dx >dmu >ws",
    "vrwkv_ddmix_fwd_bf16": "ntok T C x mu[] mm[] >out[]",
    "vrwkv_ddmix_bwd_bf16": "ntok T C x mu[] mm[] dout[] >dx >dmm[] >dmu >ws",
    "vrwkv_gn_silu_fwd_bf16": "ntok C eps y gg ln_w ln_b >out",
    "vrwkv_gn_silu_bwd_bf16": "ntok C eps y gg ln_w ln_b dout >dy >dgg >dparams >ws",
    "vrwkv_decay_fwd_bf16": "ntok C h w0 >w",
    "vrwkv_decay_bwd_bf16": "ntok C h w0 dw >dh >dw0 >ws",
    "vrwkv_kva_fwd_bf16": "ntok C has k v* vfirst* vl* al k_k k_a a0 v0* >k2 >v2* >z >b",
    "vrwkv_kva_bwd_bf16": "ntok C has k v* vfirst* vl* al k_k k_a a0 v0* dk2 dv2* dz db >dk >dv* >dvfirst* >dvl* >dal >dparams >ws",
    "vrwkv_kva_bwd2_bf16": "ntok C has k v* vfirst* vl* al k_k k_a a0 v0* dk2 dv2* dz db dk2_second? dv2_second? "
                           ">dk >dv* >dvfirst* >dvl* >dal >dparams >ws",
    "vrwkv_kva_bwd3_bf16": "ntok C has k v* vfirst* vl* al k_k k_a a0 v0* dk2 dv2* dz db dk2_second? dv2_second? dvfirst_in? "
                           ">dk >dv* >dvfirst* >dvl* >dal >dparams >ws",
    "vrwkv_post_fwd_bf16": "ntok C eps y r k v g ln_w ln_b r_k >out",
    "vrwkv_post_bwd_bf16": "ntok C eps y r k v g ln_w ln_b r_k dout >dy >dr >dk >dv >dg >dparams >ws",
    "vrwkv_relusq_fwd_bf16": "n h >y",
    "vrwkv_relusq_bwd_bf16": "n h dy >dh",
}
SCALARS = {"ntok": L, "T": I, "C": I, "M": I, "has": I, "eps": F32, "n": L}
VALID = {"ntok": 4, "T": 2, "C": 64, "M": 6, "has": 1, "eps": EPS, "n": 4 * 64}
REFUSE_BUF = 8 * 8256                  # floats per buffer: 4 rows (5 in `ragged`) of the widest C tried, 6 partial rows -- no case depends on being refused to stay in bounds


def _defects(sig):
    """The defective calls of one entry: {id: {argument: value}}, a pointer's value None (NULL) or, for an optional one, True (given);
    (array, i) addresses one element.  One defect each, then the pairs that show which check comes first."""
    args = sig.split()
    names = [a.strip(">?*[]") for a in args]
    required = [n for a, n in zip(args, names) if n not in SCALARS and not a.endswith("?")]
    arrays = [n for a, n in zip(args, names) if a.endswith("[]")]
    last = 4 if "M" not in names else 5
    novres = {"has": 0, **{n: None for a, n in zip(args, names) if a.endswith("*")}}
    d = {}
    if "ntok" in names:
        d["ntok0"] = {"ntok": 0}
    if "T" in names:
        d["T0"] = {"T": 0}
        d["ragged"] = {"ntok": 5}                          # ntok % T != 0
    if "C" in names:
        d.update({f"C{c}": {"C": c} for c in (0, 32, 8256)})
        d[f"C32+null:{required[0]}"] = {"C": 32, required[0]: None}
    d.update({f"null:{n}": {n: None} for n in required})
    for n in arrays:
        d[f"null:{n}[{last}]"] = {(n, last): None}
        d[f"C32+null:{n}[{last}]"] = {"C": 32, (n, last): None}
    if "M" in names:
        d["M3"] = {"M": 3}
    if "M" in names and "dout3_second" in names:
        d["M1+dout3_second"] = {"M": 1, "dout3_second": True}
    for opt in ("dv2_second", "dvfirst_in"):
        if opt in names:
            d[f"novres+{opt}"] = {**novres, opt: True}
    if "dv2_second" in names:
        d["ntok0+novres+dv2_second"] = {**novres, "ntok": 0, "dv2_second": True}
    # `first` together with y_prev in mix_bwd_ln (tmix_fused.hip) is EINVAL there, but no exported entry takes both: nothing to call
    if "n" in names:
        d["n0"] = {"n": 0}
        d["n%8"] = {"n": 4 * 64 + 4}
    return d


# What every entry answered before its host side was folded into one check / launch path, read off that code by running these very
# calls against it (not derived from what the codes ought to be).  NULL, a count of zero and a bad M are found before a bad shape,
# except the elements of a pointer array, which the mix and ddmix entries look at after the shape.
_MIX_ESHAPE = "ragged C0 C32 C8256 C32+null:mu[5] "
_MIX_LN_EINVAL = ("ntok0 T0 C32+null:xn null:xn null:mean null:rstd null:ln_w null:ln_b null:mu null:dout null:dx null:dmu null:ws "
                  "null:mu[5] null:dout[5] M3 M1+dout3_second")
_KVA_BWD_EINVAL = ("ntok0 C32+null:k null:k null:v null:vfirst null:vl null:al null:k_k null:k_a null:a0 null:v0 null:dk2 null:dv2 null:dz "
                   "null:db null:dk null:dv null:dvfirst null:dvl null:dal null:dparams null:ws ")
_ROW_ESHAPE = "C0 C32 C8256"
REFUSALS = {
    "vrwkv_mix_fwd_bf16": {EINVAL: "ntok0 T0 C32+null:x null:x null:mu null:out null:mu[5] null:out[5] M3",
                           ESHAPE: _MIX_ESHAPE + "C32+null:out[5]"},
    "vrwkv_mix_fwd_prev_bf16": {EINVAL: "ntok0 T0 C32+null:x null:x null:mu null:out null:mu[5] null:out[5] M3",
                                ESHAPE: _MIX_ESHAPE + "C32+null:out[5]"},
    "vrwkv_mix_bwd_bf16": {EINVAL: "ntok0 T0 C32+null:x null:x null:mu null:dout null:dx null:dmu null:ws null:mu[5] null:dout[5] M3",
                           ESHAPE: _MIX_ESHAPE + "C32+null:dout[5]"},
    "vrwkv_mix_bwd2_bf16": {EINVAL: "ntok0 T0 C32+null:x null:x null:mu null:dout null:dx null:dmu null:ws null:mu[5] null:dout[5] M3 "
                                    "M1+dout3_second",
                            ESHAPE: _MIX_ESHAPE + "C32+null:dout[5]"},
    "vrwkv_mix_bwd_ln_bf16": {EINVAL: _MIX_LN_EINVAL, ESHAPE: _MIX_ESHAPE + "C32+null:dout[5]"},
    "vrwkv_mix_bwd_ln_packed_bf16": {EINVAL: _MIX_LN_EINVAL, ESHAPE: _MIX_ESHAPE + "C32+null:dout[5]"},
    "vrwkv_mix_bwd_ln_carry_bf16": {EINVAL: _MIX_LN_EINVAL, ESHAPE: _MIX_ESHAPE + "C32+null:dout[5]"},
    "vrwkv_ddmix_fwd_bf16": {EINVAL: "ntok0 T0 C32+null:x null:x null:mu null:mm null:out null:mu[4] null:mm[4] null:out[4]",
                             ESHAPE: "ragged C0 C32 C8256 C32+null:mu[4] C32+null:mm[4] C32+null:out[4]"},
    "vrwkv_ddmix_bwd_bf16": {EINVAL: "ntok0 T0 C32+null:x null:x null:mu null:mm null:dout null:dx null:dmm null:dmu null:ws null:mu[4] "
                                     "null:mm[4] null:dout[4] null:dmm[4]",
                             ESHAPE: "ragged C0 C32 C8256 C32+null:mu[4] C32+null:mm[4] C32+null:dout[4] C32+null:dmm[4]"},
    "vrwkv_gn_silu_fwd_bf16": {EINVAL: "ntok0 C32+null:y null:y null:gg null:ln_w null:ln_b null:out", ESHAPE: _ROW_ESHAPE},
    "vrwkv_gn_silu_bwd_bf16": {EINVAL: "ntok0 C32+null:y null:y null:gg null:ln_w null:ln_b null:dout null:dy null:dgg null:dparams null:ws",
                               ESHAPE: _ROW_ESHAPE},
    "vrwkv_decay_fwd_bf16": {EINVAL: "ntok0 C32+null:h null:h null:w0 null:w", ESHAPE: _ROW_ESHAPE},
    "vrwkv_decay_bwd_bf16": {EINVAL: "ntok0 C32+null:h null:h null:w0 null:dw null:dh null:dw0 null:ws", ESHAPE: _ROW_ESHAPE},
    "vrwkv_kva_fwd_bf16": {EINVAL: "ntok0 C32+null:k null:k null:v null:vfirst null:vl null:al null:k_k null:k_a null:a0 null:v0 null:k2 "
                                   "null:v2 null:z null:b",
                           ESHAPE: _ROW_ESHAPE},
    "vrwkv_kva_bwd_bf16": {EINVAL: _KVA_BWD_EINVAL, ESHAPE: _ROW_ESHAPE},
    "vrwkv_kva_bwd2_bf16": {EINVAL: _KVA_BWD_EINVAL + "novres+dv2_second ntok0+novres+dv2_second", ESHAPE: _ROW_ESHAPE},
    "vrwkv_kva_bwd3_bf16": {EINVAL: _KVA_BWD_EINVAL + "novres+dv2_second novres+dvfirst_in ntok0+novres+dv2_second", ESHAPE: _ROW_ESHAPE},
    "vrwkv_post_fwd_bf16": {EINVAL: "ntok0 C32+null:y null:y null:r null:k null:v null:g null:ln_w null:ln_b null:r_k null:out",
                            ESHAPE: _ROW_ESHAPE},
    "vrwkv_post_bwd_bf16": {EINVAL: "ntok0 C32+null:y null:y null:r null:k null:v null:g null:ln_w null:ln_b null:r_k null:dout null:dy "
                                    "null:dr null:dk null:dv null:dg null:dparams null:ws",
                            ESHAPE: _ROW_ESHAPE},
    "vrwkv_relusq_fwd_bf16": {EINVAL: "null:h null:y n0", ESHAPE: "n%8"},
    "vrwkv_relusq_bwd_bf16": {EINVAL: "null:h null:dy null:dh n0", ESHAPE: "n%8"},
}


def _entry_rc(be, name, zeros, outs, change):
    """The code of one call of `name`: the VALID scalars, every required pointer given -- `zeros` for what the entry reads, a row of
    `outs` each for what it writes --, then `change` applied (see _defects)."""
    vals, types, k = [], [], 0
    for a in GLUE_ENTRIES[name].split():
        n = a.strip(">?*[]")
        if n in SCALARS:
            vals.append(change.get(n, VALID[n]))
            types.append(SCALARS[n])
            continue
        ptrs = []
        for i in range(6 if a.endswith("[]") else 1):
            ptrs.append(outs[k].data_ptr() if a.startswith(">") else zeros.data_ptr())
            k += a.startswith(">")
            if (n, i) in change:
                ptrs[i] = None
        if not change.get(n, not a.endswith("?")):
            vals.append(None)
        else:
            vals.append((VP * 6)(*ptrs) if a.endswith("[]") else VP(ptrs[0]))
        types.append(VP)
    return be.rc(name, types, *vals)


@pytest.mark.parametrize("backend", BACKENDS)
def test_glue_entries_refuse_in_order(backend, be):
    """Every entry answers every defective call of _defects with the code of REFUSALS and launches nothing: what it would write is NaN
    before the call and after it.  The call without a defect then runs."""
    zeros = torch.zeros(REFUSE_BUF, dtype=torch.float32, device=be.dev)
    outs = torch.full((12, REFUSE_BUF), float("nan"), dtype=torch.float32, device=be.dev)
    assert set(REFUSALS) == set(GLUE_ENTRIES)
    for name, sig in GLUE_ENTRIES.items():
        want = {d: code for code, ds in REFUSALS[name].items() for d in ds.split()}
        defects = _defects(sig)
        assert set(want) == set(defects), name
        for did, change in defects.items():
            rc = _entry_rc(be, name, zeros, outs, change)
            assert rc == want[did], (name, did, rc)
            assert bool(torch.isnan(outs).all()), (name, did, "a refused call wrote")
        assert _entry_rc(be, name, zeros, outs, {}) == 0, name
        outs.fill_(float("nan"))


def _same_results(runs, tag):
    """Every run's buffers written up to their guard rows and bit for bit those of the first run."""
    for res in runs:
        written(res, None, 0)
    for res in runs[1:]:
        for name in runs[0]:
            assert torch.equal(bits(res[name]), bits(runs[0][name])), f"{tag} {name}: the forwarding entry differs from the full one"


@pytest.mark.parametrize("backend,sid", [c for c in _cases() if c.values[1] in FULL_MATRIX])
def test_forwarding_entries_are_the_full_entry(backend, be, sid):
    """The entries that only forward -- mix_fwd, mix_bwd, kva_bwd, kva_bwd2 -- and the three mix_bwd_ln entries with their optional
    pointers NULL: bit for bit (outputs and fp32 parameter gradients) the entry they forward to."""
    B, T, C = be.shape(sid)
    ntok = B * T
    g = be.gen(19 * ntok + C)
    x = rnd(be, g, ntok, C)
    for M in (1, 2, 6):
        mus, douts = [unif(be, g, C) for _ in range(M)], [rnd(be, g, ntok, C) for _ in range(M)]
        runs = []
        for prev in (False, True):
            outs = [nan_rows(be, ntok, C) for _ in range(M)]
            if prev:
                be.call("vrwkv_mix_fwd_prev_bf16", [L, I, I, I] + [VP] * 4, ntok, T, C, M, P(x), None, PA(mus), PA(outs))
            else:
                be.call("vrwkv_mix_fwd_bf16", [L, I, I, I] + [VP] * 3, ntok, T, C, M, P(x), PA(mus), PA(outs))
            runs.append({f"out{j}": o for j, o in enumerate(outs)})
        _same_results(runs, f"mix_fwd/{sid}/M{M}")
        runs = []
        for full in (False, True):
            dx, dmu, ws = nan_rows(be, ntok, C), nan_rows(be, M, C, torch.float32), nan_ws(be, ntok, C, M)
            if full:
                be.call("vrwkv_mix_bwd2_bf16", [L, I, I, I] + [VP] * 7, ntok, T, C, M, P(x), PA(mus), PA(douts), None, P(dx), P(dmu), P(ws))
            else:
                be.call("vrwkv_mix_bwd_bf16", [L, I, I, I] + [VP] * 6, ntok, T, C, M, P(x), PA(mus), PA(douts), P(dx), P(dmu), P(ws))
            runs.append({"dx": dx, "dmu": dmu})
        _same_results(runs, f"mix_bwd/{sid}/M{M}")

    # mix_bwd_ln (M = 6), with and without the second gradient of output 3
    mean, rstd = torch.randn(ntok, generator=g, device=be.dev) * 0.1, torch.rand(ntok, generator=g, device=be.dev) + 0.5
    ln_w, ln_b = rnd(be, g, C, scale=0.5, shift=1.0), rnd(be, g, C, scale=0.1)
    for d3b in (None, rnd(be, g, ntok, C)):
        runs = []
        for entry, nulls in (("vrwkv_mix_bwd_ln_bf16", 0), ("vrwkv_mix_bwd_ln_packed_bf16", 1), ("vrwkv_mix_bwd_ln_carry_bf16", 3)):
            dx, dmu, ws = nan_rows(be, ntok, C), nan_rows(be, 6, C, torch.float32), nan_ws(be, ntok, C, 6)
            be.call(entry, [L, I, I, I] + [VP] * (11 + nulls), ntok, T, C, 6, P(x), P(mean), P(rstd), P(ln_w), P(ln_b), PA(mus), PA(douts),
                    P(d3b), *[None] * nulls, P(dx), P(dmu), P(ws))
            runs.append({"dx": dx, "dmu": dmu})
        _same_results(runs, f"mix_bwd_ln/{sid}/{'dup3' if d3b is not None else 'plain'}")

    k, v, vf, vl, al = [rnd(be, g, ntok, C) for _ in range(5)]
    k_k, k_a, a0, v0 = [rnd(be, g, C, scale=0.5) for _ in range(4)]
    dk2, dv2, dz, db = [rnd(be, g, ntok, C) for _ in range(4)]
    for vres in (False, True):
        ins = [P(t) if vres or i not in (1, 2, 3, 8, 10) else None for i, t in enumerate((k, v, vf, vl, al, k_k, k_a, a0, v0, dk2, dv2, dz, db))]
        runs = []
        for entry, nulls in (("vrwkv_kva_bwd_bf16", 0), ("vrwkv_kva_bwd2_bf16", 2), ("vrwkv_kva_bwd3_bf16", 3)):
            bw = {n: nan_rows(be, ntok, C) for n in (("dk", "dv", "dvfirst", "dvl", "dal") if vres else ("dk", "dal"))}
            pg, ws = nan_rows(be, 4, C, torch.float32), nan_ws(be, ntok, C, 4)
            be.call(entry, [L, I, I] + [VP] * (20 + nulls), ntok, C, int(vres), *ins, *[None] * nulls,
                    P(bw["dk"]), P(bw.get("dv")), P(bw.get("dvfirst")), P(bw.get("dvl")), P(bw["dal"]), P(pg), P(ws))
            runs.append({**bw, "dparams": pg})
        _same_results(runs, f"kva_bwd/{sid}/{'vres' if vres else 'novres'}")
