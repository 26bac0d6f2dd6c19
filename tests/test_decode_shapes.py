"""The one-token decode step -- csrc/gemv_decode.hip (batched GEMV, its copy side job, the LayerNorm fold), csrc/decode_fused.hip
(ln_mix_prev, tmix_head) and csrc/wkv7_step.hip -- at the widths and batch sizes where the kernels change their code path, through the
C ABI, on two backends with the same test bodies: the host lockstep emulator (tests/emu/emu_gemv_decode.cpp, emu_decode_fused.cpp and
emu_wkv7_step.cpp compile the .hip files whole: CPU tensors, no marker) and the product library (CUDA tensors, `gpu` marker).

What picks the path (the tables GEMV_K, FOLD_K, LNMIX_C, HEAD_BH and HEAD_D below say what every id reaches).  gemv_multi: K < 512
walks a row with a group of G = 2^floor(log2(min(K / 8, 32))) lanes, 64 / G rows at a time, 8 rows per wave, 32 per workgroup, x staged
in LDS sized by the widest short job; K >= 512 gives a wave 2 rows and batches of 256 chunks (8 rows per workgroup); K > 2048 with
K % 32 == 0 splits a row over the four waves (2 rows per workgroup, quarter kq = K / 32 chunks).  Every case lays its N values
(all of the path's list) as the jobs of ONE launch, so find_job and wg_begin are walked at ragged boundaries everywhere, every job
with its own activation and residual; one-job launches ride along.  The LayerNorm fold is compiled for 1 or 2 chunks per thread
(K > 2048) and 1, 2 or 4 batch rows; ln_mix_prev owns up to 4 chunks per thread; tmix_head walks D / 32 chunks per quarter of each
LoRA width.

References: plain torch in fp64 on the backend's device, written from src/model.py:166-194,222-223,250-253 of the reference.
  GEMV       act(x W^T) + res
  fold       h = bf16(LN64(x)),  in_j = bf16(h + (x_prev - h) mu_j)  (the kernel parks it in LDS as bf16),  y_j = act(in_j W_j^T)
  ln_mix     h = bf16(LN64(x)),  out_j = h + (x_prev - h) mu_j rounded once
  tmix_head  model.py:176-193 at T = 1 with a bf16 rounding where the kernel's comments place one -- lo_i, w_raw, k2, v2, -kk, kk a,
             y -- the recurrence as oracle.wkv7_oracle.wkv7_naive states it, the GroupNorm in elementary ops (see test_glue_shapes.py)
  wkv7_step  oracle.wkv7_oracle.wkv7_naive in fp64
Every case asserts: return code 0; pure outputs are NaN before the call and every output buffer ends in a guard row -- results finite,
guards untouched; a second call on the same inputs is bit-identical.  The argument rejections (test_rejects_*) assert the exact VRWKV_E*
code and that the NaN outputs are untouched, on both backends.

Bounds.
  Results with a single rounding (GEMV y, h, ln_mix's outputs): tests.parity.bf16_close against the reference rounded once, tol 1e-3,
  flips < 0.01 (FLIP_Y of the project), evaluated over all launches of a case (a case of the split-K path has 11 rows per batch row:
  one tie would be 9 % of one launch).  tests.parity.group_bias on every GEMV output of at least 64 elements and on each case's total.
  The outlier rows are evaluated over the channels other than the outlier.
  Chains with intermediate roundings (the fold's y, tmix_head's out and fp32 state): rel-RMS against the fp64 chain (bf16 results
  against its value rounded once).  The floor is the same staged reference evaluated in fp32 torch, and again with every exp, log and
  rsqrt result moved up by one fp32 ulp (the hardware's 1-ulp transcendentals), against the fp64 one, on the CPU, worst over all
  cases; the bound is 4 x that floor, capped by what tests/test_stateful_gpu.py asserts (8e-3, 1e-2, 2e-3).  VRWKV_TEST_NOTES=1 prints
  every figure, the floors included.
  Floors (worst case of the fp32 staged reference | of the same with nudged exp / log / rsqrt), the bound, the worst kernel figure:
    fold y      5.88e-05 | 1.62e-03 (K2056-B2 one job: 18 elements)  ->  6.5e-3   emulator 3.27e-04 (K4096-B4 8 jobs), MI355X 5.17e-04 (K1000-B3 8 jobs)
    tmix out    4.97e-04 | 1.25e-03 (B2H5-D96-later)                 ->  5.0e-3   emulator 4.97e-04 (B5H2-D96-first), MI355X 0 (every element is the
                                                                                  rounded reference)
    tmix state  4.33e-06 | 1.36e-04 (B2H5-D96-later)                 ->  5.4e-4   emulator 1.65e-05 (B5H2-D96-later), MI355X 3.6e-08
  A floor is a handful of intermediate ties (one flipped lo_w moves a state column by up to 7e-4), so it is spiky; what the rel-RMS
  bound cannot see in tmix_head's decay is asserted per column on a head with k = 0 (test_tmix_head).
  Single roundings, worst flips: emulator 1.9e-3 (fold K520-B1 h: one element of 520), MI355X 5e-4 (gemv long K4104); on the row edges
  6.0e-3 (fold K1000 mean300, emulator) and 6.3e-3 (ln_mix C2056 mean300, MI355X): a plain fp32 sum of 300 +- 4 over the row.

The folded LayerNorm on rows whose first element is the outlier ([1000, N(0, 1) ..], [30000, N(0, 4^2) ..]), flips of h over the other
channels.  gemv_ln_kernel used to take its statistics in one pass around the row's first element; a CPU simulation of that arithmetic had
given 2.6 % at K = 2048 and 8.2 % at K = 4096 for the first row.  That kernel on the emulator, outlier 1000 / 30000:
    K1000 1.00 % / 1.40 %    K2048 2.64 % / 0.68 %    K2056 0.19 % / 0.92 %    K4096 5.23 % / 2.71 %     (limit 1 %; outlier last: <= 0.05 %)
and on the MI355X (outlier 1000):  K1000 1.20 %, K2048 2.74 %, K2056 0.97 % (1.41 % for 30000), K4096 1.66 %.
The kernel now takes the mean first and the variance around it, as ln_mix_prev_kernel does: 0 on the emulator and at most 0.05 % on the
MI355X for all four outlier rows at every K; mean 300 stays at or below 0.6 %, the constant row gives h == ln_b bit for bit.
"""
import math

import pytest
import torch

from oracle.wkv7_oracle import wkv7_naive
from tests.parity import NOTES, group_bias
from tests.shape_checks import Checks
from tests.test_glue_shapes import F32, I, L, P, VP, Backend, bits, nan_rows, rnd, same_bits, unif, written

EPS_LN, EPS_GN = 1e-5, 64e-5
TOL = 1e-3
FLIP = {"emu": 0.01, "hip": 0.01}              # the project's limit for a result that is rounded once (FLIP_Y)
CHAIN = {"fold_y": 6.5e-3, "tmix_out": 5.0e-3, "tmix_state": 5.4e-4}       # 4 x the worst floor (module docstring)
CHAIN_CAP = {"fold_y": 8e-3, "tmix_out": 1e-2, "tmix_state": 2e-3}         # tests/test_stateful_gpu.py
EINVAL, ESHAPE, EALIGN = -1, -2, -3

BACKENDS = ["emu", pytest.param("hip", marks=pytest.mark.gpu)]
# gemv_multi        K      what it reaches
GEMV_K = {
    "short": [     # 32 rows per workgroup, 8 per wave
        (8,     "G = 1: one lane per row, 64 rows at once of which 8 live"),
        (16,    "G = 2"),
        (24,    "G = 2 with a ragged second trip (3 chunks)"),
        (32,    "G = 4, 16 rows at once"),
        (64,    "G = 8, exactly the wave's 8 rows at once"),
        (96,    "G = 8 with a second trip of 4 live lanes"),
        (128,   "G = 16, 4 rows at once"),
        (256,   "G = 32, 2 rows at once, one trip"),
        (504,   "G = 32, the widest short row: a ragged second trip (63 chunks)"),
    ],
    "long": [      # 8 rows per workgroup, 2 per wave
        (512,   "the narrowest long row: 64 chunks, q = 0 only"),
        (520,   "the tail c < kchunks in q = 1 (one live lane)"),
        (2048,  "one full batch of 256 chunks"),
        (2056,  "a second trip of the batch loop with one live lane"),
        (4104,  "K > 2048 unsplit (K % 32 != 0): three trips, the last with one lane"),
    ],
    "split": [     # 2 rows per workgroup, a quarter of the row per wave
        (2080,  "kq = 65: q = 1 with one live lane"),
        (4096,  "kq = 128"),
        (8192,  "kq = 256: one full batch per wave"),
        (8224,  "kq = 257: a second trip with one live lane"),
    ],
}
GEMV_N = {"short": (1, 8, 9, 31, 32, 33, 70), "long": (1, 2, 7, 8, 9, 17), "split": (1, 2, 3, 5)}      # against 32 / 8 / 2 rows per workgroup
GEMV_ALL_B = {"short": 24, "long": 2056, "split": 8224}         # every B in 1..4 here, B in {1, 4} elsewhere
# gemv_ln_multi
FOLD_K = [
    (512,   "CH = 1, two waves of threads live"),
    (520,   "CH = 1, one lane of wave 1 live; the row walk's tail"),
    (1000,  "CH = 1, 125 chunks: waves 2 and 3 contribute 0 to the statistics"),
    (2048,  "CH = 1 full"),
    (2056,  "CH = 2: the first thread alone owns a second chunk"),
    (4096,  "CH = 2 full, the widest row the fold admits"),
]
FOLD_N8 = (9, 1, 300, 9, 1, 9, 1, 9)           # 8 jobs, ragged against 8 rows per workgroup; job 0 has two workgroups, only the first writes h
FOLD_EMU_WIDE_N = 40                            # the emulator's 300 at K >= 2048
# decode_ln_mix
LNMIX_C = [
    (8,     "one chunk: one live thread"),
    (64,    "8 threads"),
    (2040,  "the last chunk of the first of LM_MAXCH trips"),
    (2048,  "the first trip full"),
    (2056,  "the first overflow into trip 2"),
    (8192,  "the cap: 4 chunks per thread"),
]
# tmix_head
HEAD_BH = [(1, 1), (2, 5), (4, 3), (5, 2)]      # one head; an odd H; B = 4; B past the GEMV cap (this entry has none)
HEAD_D = {                                      # LoRA widths (w, a, g, v-gate): D / 32 chunks per quarter
    "D32":  (32, 32, 32, 32),                   # one chunk each (the C = 256 model)
    "D96":  (96, 64, 160, 32),                  # 3, 2, 5, 1: the unrolled-by-4 loop with a remainder, different widths in one call
    "D256": (256, 128, 96, 64),                 # 8, 4, 3, 2 (the C >= 2048 models)
}

CHECKS = Checks("decode", FLIP, {"emu": 0.0, "hip": 0.0}, TOL)
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
        print(f"[decode] {be.name} {name}: {kind} rel-RMS {err:.3e}   (worst so far {WORST.get(key, (0.0, ''))[0]:.3e} {WORST.get(key, (0.0, ''))[1]})")
    assert CHAIN[kind] <= CHAIN_CAP[kind]
    assert err < CHAIN[kind], f"{name}: {kind} rel-RMS {err:.3e} >= {CHAIN[kind]:.1e}"


# ------------------------------------------------------------------------------------------------ references
class Ops:
    """The arithmetic of a staged reference: fp64, or fp32 with (nudge) every exp / log / rsqrt result one ulp up, for the floors."""
    def __init__(self, dt=torch.float64, nudge=False):
        self.dt, self.nudge = dt, nudge

    def t(self, x):
        return None if x is None else x.to(self.dt)

    def up(self, x):
        return torch.nextafter(x, torch.full_like(x, math.inf)) if self.nudge else x

    def exp(self, x):
        return self.up(torch.exp(x))

    def log(self, x):
        return self.up(torch.log(x))

    def rsqrt(self, x):
        return self.up(torch.rsqrt(x))

    def sigmoid(self, x):
        return 1 / (1 + self.exp(-x))

    def rb(self, x):
        return x.float().bfloat16().to(self.dt)

    def act(self, v, act):
        return [v, 1 - 2 / (1 + self.exp(2 * v)), self.sigmoid(v), torch.relu(v) ** 2][act]


O64 = Ops()


def act64(v, act):
    return [v, torch.tanh(v), torch.sigmoid(v), torch.relu(v) ** 2][act]


def ref_ln(o, x, lw, lb, eps=EPS_LN):
    """bf16(LayerNorm(x)) over the last dimension, biased variance, in elementary ops."""
    x = o.t(x)
    d = x - x.mean(-1, keepdim=True)
    return o.rb(d * o.rsqrt((d * d).mean(-1, keepdim=True) + eps) * o.t(lw) + o.t(lb))


def ref_fold(o, x, lw, lb, prev, jobs):
    """jobs: (W, mu, act).  Returns h and the y_j."""
    h = ref_ln(o, x, lw, lb)
    return h, [o.act(o.rb(h + (o.t(prev) - h) * o.t(mu)) @ o.t(W).t(), act) for W, mu, act in jobs]


def ref_tmix(o, B, H, r, k, v, vf, hid, W2t, w0, a0, v0, k_k, k_a, r_k, ln_w, ln_b, S):
    """src/model.py:176-193 for one token; returns out (B, C) and the new state (B, H, 64, 64) [value row][key column]."""
    t, hd = o.t, lambda x: x.view(-1, H, 64)
    r, k, v, vf = t(r), t(k), t(v), t(vf)
    lo = [o.rb(t(h) @ t(W).t()) for h, W in zip(hid, W2t)]
    u = lo[0] + t(w0)
    w_raw = o.rb(-(torch.clamp(-u, min=0) + o.log(1 + o.exp(-u.abs()))) - 0.5)       # -softplus(-u) - 0.5
    a = o.sigmoid(t(a0) + lo[1])
    kk = hd(k * t(k_k))
    kk = kk / kk.pow(2).sum(-1, keepdim=True).sqrt().clamp_min(1e-12)                # F.normalize
    k2 = hd(o.rb(k * (1 + (a - 1) * t(k_a))))
    v2 = hd(o.rb(v + (vf - v) * o.sigmoid(t(v0) + lo[3])) if vf is not None else v)
    z, b = o.rb(-kk), o.rb(kk * hd(a))
    decay = hd(o.exp(-o.exp(w_raw)))
    S, rh = t(S), hd(r)
    sa = (S * z[:, :, None, :]).sum(-1)
    S = S * decay[:, :, None, :] + sa[..., None] * b[:, :, None, :] + v2[..., None] * k2[:, :, None, :]
    y = o.rb((S * rh[:, :, None, :]).sum(-1))
    dlt = y - y.mean(-1, keepdim=True)
    rstd = o.rsqrt((dlt * dlt).mean(-1, keepdim=True) + EPS_GN)
    sb = (rh * k2 * hd(t(r_k))).sum(-1, keepdim=True)
    out = (dlt * rstd * hd(t(ln_w)) + hd(t(ln_b)) + sb * v2) * hd(lo[2])
    return out.reshape(B, H * 64), S


def floors(name, fn, kinds):
    """fn(ops) -> {kind: tensor}: the fp32 evaluations of a staged reference against the fp64 one (VRWKV_TEST_NOTES=1, CPU inputs)."""
    if not NOTES:
        return
    want = fn(O64)
    for label, o in (("fp32", Ops(torch.float32)), ("fp32 nudged", Ops(torch.float32, True))):
        got = fn(o)
        for kind in kinds:
            g, w = got[kind], want[kind]
            if kind != "tmix_state":
                g, w = rb64(g), rb64(w)
            print(f"[decode] floor {name} {label}: {kind} rel-RMS {rel_rms(g, w):.3e}")


# ------------------------------------------------------------------------------------------------ gemv_multi
def gemv_jobs(be, g, B, shapes, rot=0):
    """One job per (N, K): W ~ N(0, 1 / K), x ~ N(0, 1); job i gets activation (i + rot) % 4 and a residual where bit 2 of i + rot is set."""
    jobs = []
    for i, (N, K) in enumerate(shapes):
        jobs.append(dict(W=rnd(be, g, N, K, scale=K ** -0.5), x=rnd(be, g, B, K), act=(i + rot) % 4,
                         res=rnd(be, g, B, N) if (i + rot) & 4 else None))
    return jobs


def run_gemv(be, B, jobs, copy=None):
    """One launch; returns the (B + 1, N_j) outputs, NaN before the call, the last row a guard."""
    ys = [nan_rows(be, B, j["W"].shape[0]) for j in jobs]
    args = [len(jobs), B, arr([j["W"] for j in jobs]), arr([j["x"] for j in jobs]), arr([j["res"] for j in jobs]), arr(ys),
            ints([j["W"].shape[0] for j in jobs]), ints([j["W"].shape[1] for j in jobs]), ints([j["act"] for j in jobs])]
    if copy is None:
        be.call("vrwkv_gemv_multi_bf16", [I, I] + [VP] * 7, *args)
    else:
        src, dst, elems = copy
        be.call("vrwkv_gemv_multi_copy_bf16", [I, I] + [VP] * 9 + [L], *args, P(src), P(dst), elems)
    written({f"y{j}": y for j, y in enumerate(ys)}, None, 0)
    return ys


def ref_gemv(B, j):
    v = act64(j["x"].double() @ j["W"].double().t(), j["act"])
    return v + j["res"].double() if j["res"] is not None else v


def check_gemv(be, launches, tag):
    """launches: (B, jobs, ys).  group_bias per output of >= 64 elements; bf16_close and group_bias over the case's total."""
    got, want = [], []
    for B, jobs, ys in launches:
        for j, y in zip(jobs, ys):
            ref = ref_gemv(B, j)
            got.append(y[:-1].reshape(-1))
            want.append(ref.reshape(-1))
            if ref.numel() >= 64:
                group_bias(y[:-1], ref, f"{tag} B{B} N{ref.shape[1]} K{j['W'].shape[1]} act{j['act']}")
    got, want = torch.cat(got), torch.cat(want)
    CHECKS.act(be, got, want, tag, guard=False)
    group_bias(got, want, tag)


@pytest.mark.parametrize("backend,path,K", _params([(p, K) for p in GEMV_K for K, _ in GEMV_K[p]]))
def test_gemv(backend, be, path, K):
    """Every N of the path as the jobs of one launch, every activation with and without a residual at every N (8 rotations), plus a
    launch of one job; B in 1..4 at GEMV_ALL_B, else {1, 4}."""
    g = be.gen(K)
    launches = []
    for B in ((1, 2, 3, 4) if K == GEMV_ALL_B[path] else (1, 4)):
        for rot in range(8):
            jobs = gemv_jobs(be, g, B, [(N, K) for N in GEMV_N[path]], rot)
            ys = run_gemv(be, B, jobs)
            if rot == 0:
                same_bits(dict(enumerate(ys)), dict(enumerate(run_gemv(be, B, jobs))))
            launches.append((B, jobs, ys))
        one = gemv_jobs(be, g, B, [(GEMV_N[path][-1], K)], rot=1 + B)
        launches.append((B, one, run_gemv(be, B, one)))
    check_gemv(be, launches, f"gemv/{path}/K{K}")


# 8 jobs (GV_MAX_JOBS) over the three paths: the LDS size follows the widest short job (504), which is not the first; every N is
# ragged against its path's rows per workgroup, so every wg_begin falls behind a partly filled workgroup
MIXED = [(33, 64), (9, 520), (3, 2080), (70, 504), (17, 2056), (5, 8224), (31, 8), (1, 24)]


@pytest.mark.parametrize("backend,B", _params([1, 2, 3, 4]))
def test_gemv_mixed_paths(backend, be, B):
    g = be.gen(77 + B)
    launches = []
    for rot in range(8):
        jobs = gemv_jobs(be, g, B, MIXED, rot)
        ys = run_gemv(be, B, jobs)
        if rot == 0:
            same_bits(dict(enumerate(ys)), dict(enumerate(run_gemv(be, B, jobs))))
        launches.append((B, jobs, ys))
    check_gemv(be, launches, f"gemv/mixed/B{B}")


@pytest.mark.parametrize("backend,B", _params([1, 4]))
def test_gemv_saturated(backend, be, B):
    """Pre-activations of exactly +-100 (+-130 on the split path): fast_exp over- and underflows; tanh and sigmoid give their limits."""
    for K, wv in ((64, 1.5625), (512, 0.1953125), (2080, 0.0625)):
        N = 9
        sign = torch.tensor([1.0 if n % 2 == 0 else -1.0 for n in range(N)], device=be.dev)
        W = (sign[:, None] * torch.full((N, K), wv, device=be.dev)).bfloat16()
        x = torch.ones(B, K, dtype=torch.bfloat16, device=be.dev)
        jobs = [dict(W=W, x=x, act=a, res=None) for a in (1, 2)]
        yt, ys = run_gemv(be, B, jobs)
        assert torch.equal(yt[:-1].float(), sign.expand(B, N)), f"tanh at +-{wv * K}"
        assert torch.equal(ys[:-1].float(), ((sign + 1) / 2).expand(B, N)), f"sigmoid at +-{wv * K}"
        for j, y in zip(jobs, (yt, ys)):
            assert torch.equal(y[:-1].float(), rb64(ref_gemv(B, j)).float())


@pytest.mark.parametrize("backend,elems", _params([0, 8, 2048, 2056, 4 * 4096]))
def test_gemv_copy(backend, be, elems):
    """The copy side job of workgroup 0: 2048 elements are one vector per thread, 2056 one more for thread 0."""
    B = 3
    g = be.gen(elems + 5)
    jobs = gemv_jobs(be, g, B, [(9, 520), (33, 64), (3, 2080)], rot=5)
    src = rnd(be, g, elems + 8)
    dst = torch.full((elems + 8,), float("nan"), dtype=torch.bfloat16, device=be.dev)
    plain = run_gemv(be, B, jobs)
    ys = run_gemv(be, B, jobs, copy=(src if elems else None, dst if elems else None, elems))
    assert torch.equal(bits(dst[:elems]), bits(src[:elems])), "dst differs from src"
    assert bool(torch.isnan(dst[elems:].float()).all()), "written past copy_elems"
    same_bits(dict(enumerate(ys)), dict(enumerate(plain)))
    check_gemv(be, [(B, jobs, ys)], f"gemv/copy{elems}")


# ------------------------------------------------------------------------------------------------ gemv_ln_multi
def ln_params(be, g, K):
    return rnd(be, g, K, scale=0.2, shift=1.0), rnd(be, g, K, scale=0.1)


def run_fold(be, B, K, x, lw, lb, prev, jobs):
    h, ys = nan_rows(be, B, K), [nan_rows(be, B, W.shape[0]) for W, _, _ in jobs]
    keep = prev.clone()
    be.call("vrwkv_gemv_ln_multi_bf16", [I, I, I, VP, VP, VP, VP, F32] + [VP] * 6, len(jobs), B, K, arr([W for W, _, _ in jobs]), P(x), P(lw),
            P(lb), EPS_LN, P(prev), arr([mu for _, mu, _ in jobs]), P(h), arr(ys), ints([W.shape[0] for W, _, _ in jobs]),
            ints([a for _, _, a in jobs]))
    res = {"h": h, **{f"y{j}": y for j, y in enumerate(ys)}}
    written(res, None, 0)                       # h is complete although only workgroup 0 (of job 0) writes it
    assert torch.equal(bits(prev), bits(keep)), "x_prev changed"
    return res


def fold_jobs(be, g, K, Ns, rot=0):
    return [(rnd(be, g, N, K, scale=K ** -0.5), unif(be, g, K), (j + rot) % 4) for j, N in enumerate(Ns)]


def check_fold(be, res, x, lw, lb, prev, jobs, tag, cols=None):
    h, ys = ref_fold(O64, x, lw, lb, prev, jobs)
    for b in range(x.shape[0]) if cols is not None else ():
        CHECKS.act(be, res["h"][b, cols[b]], h[b, cols[b]], f"{tag} h row {b}", guard=False)
    if cols is None:
        CHECKS.act(be, res["h"], h, f"{tag} h")
    chain(be, "fold_y", torch.cat([res[f"y{j}"][:-1].reshape(-1) for j in range(len(jobs))]), torch.cat([y.reshape(-1) for y in ys]), f"{tag} y")
    if be.name == "emu":
        floors(tag, lambda o: {"fold_y": torch.cat([y.reshape(-1) for y in ref_fold(o, x, lw, lb, prev, jobs)[1]])}, ["fold_y"])
    for j, y in enumerate(ys):
        if y.numel() >= 64:
            group_bias(res[f"y{j}"][:-1], y, f"{tag} y{j}")


@pytest.mark.parametrize("backend,K,B", _params([(K, B) for K, _ in FOLD_K for B in (1, 2, 3, 4)]))
def test_fold(backend, be, K, B):
    """8 jobs with their own mu, activation and ragged N, and a launch of one job; the row has a mean of 3 (as the model's residual)."""
    g = be.gen(10 * K + B)
    x, prev = rnd(be, g, B, K, scale=2.0, shift=3.0), rnd(be, g, B, K)
    lw, lb = ln_params(be, g, K)
    Ns = [FOLD_EMU_WIDE_N if N == 300 and be.name == "emu" and K >= 2048 else N for N in FOLD_N8]
    for tag, jobs in (("8jobs", fold_jobs(be, g, K, Ns, rot=B)), ("1job", fold_jobs(be, g, K, [9], rot=K // 8))):
        res = run_fold(be, B, K, x, lw, lb, prev, jobs)
        same_bits(res, run_fold(be, B, K, x, lw, lb, prev, jobs))
        check_fold(be, res, x, lw, lb, prev, jobs, f"fold/K{K}-B{B}/{tag}")


def edge_rows(be, g, K):
    """(name, row, channels to evaluate): a large mean, zero variance, an outlier in channel 0 (the pivot of a shifted-sum
    LayerNorm) and the same outlier in the last channel as the control."""
    every = torch.arange(K, device=be.dev)
    rows = [("mean300", rnd(be, g, K, scale=4.0, shift=300.0), every), ("const", torch.full((K,), 1.5, dtype=torch.bfloat16, device=be.dev), every)]
    for big, std in ((1000.0, 1.0), (30000.0, 4.0)):
        for at in (0, K - 1):
            r = rnd(be, g, K, scale=std)
            r[at] = big
            rows.append((f"out{big:.0f}_{'first' if at == 0 else 'last'}", r, every[every != at]))
    return rows


@pytest.mark.parametrize("backend,K", _params([1000, 2048, 2056, 4096]))
def test_fold_row_edges(backend, be, K):
    g = be.gen(K + 1)
    rows = edge_rows(be, g, K)
    lw, lb = ln_params(be, g, K)
    jobs = fold_jobs(be, g, K, [9, 70, 1], rot=1)
    for part in (rows[:3], rows[3:]):           # B = 3 twice: BB = 4 with a dead batch row; test_fold has B = 4
        B = len(part)
        x, prev = torch.stack([r for _, r, _ in part]), rnd(be, g, B, K)
        res = run_fold(be, B, K, x, lw, lb, prev, jobs)
        check_fold(be, res, x, lw, lb, prev, jobs, f"fold/edges/K{K}/{'+'.join(n for n, _, _ in part)}", cols=[c for _, _, c in part])
        for b, (name, _, _) in enumerate(part):
            if name == "const":
                assert torch.equal(bits(res["h"][b]), bits(lb)), "zero variance: h is ln_b"


# ------------------------------------------------------------------------------------------------ decode_ln_mix
def run_ln_mix(be, B, C, x, lw, lb, prev, mus):
    carried = nan_rows(be, B, C)
    carried[:-1] = prev
    outs = [nan_rows(be, B, C) for _ in mus]
    be.call("vrwkv_decode_ln_mix_bf16", [I, I, I, VP, VP, VP, F32, VP, VP, VP], B, C, len(mus), P(x), P(lw), P(lb), EPS_LN, P(carried),
            arr(mus), arr(outs))
    res = {"h": carried, **{f"out{j}": o for j, o in enumerate(outs)}}
    written(res, None, 0)
    return res


@pytest.mark.parametrize("backend,C", _params([C for C, _ in LNMIX_C]))
def test_ln_mix(backend, be, C):
    """M in {1, 6}, B in {1, 5}; narrow rows are repeated with fresh data until a case holds about 1000 elements per tensor."""
    g = be.gen(C)
    got, want = {}, {}
    for B in (1, 5):
        for M in (1, 6):
            for rep in range(max(1, 1024 // (B * C))):
                x, prev = rnd(be, g, B, C, scale=2.0, shift=0.3), rnd(be, g, B, C)
                lw, lb = ln_params(be, g, C)
                mus = [unif(be, g, C) for _ in range(M)]
                res = run_ln_mix(be, B, C, x, lw, lb, prev, mus)
                if rep == 0:
                    same_bits(res, run_ln_mix(be, B, C, x, lw, lb, prev, mus))
                h = ref_ln(O64, x, lw, lb)
                ref = {"h": h, **{f"out{j}": h + (prev.double() - h) * mu.double() for j, mu in enumerate(mus)}}
                for n in ref:
                    key = "h" if n == "h" else "out"
                    got.setdefault(key, []).append(res[n][:-1].reshape(-1))
                    want.setdefault(key, []).append(ref[n].reshape(-1))
            # mu = 1: the old carried row, bit for bit (|prev| >= 0.5 keeps fma(prev - h, 1, h) on prev); mu = 0: h, bit for bit
            prev = (prev.float().sign() * (prev.float().abs() + 0.5)).bfloat16()
            prev[prev == 0] = 0.5
            for val in (1.0, 0.0):
                res = run_ln_mix(be, B, C, x, lw, lb, prev, [torch.full((C,), val, dtype=torch.bfloat16, device=be.dev)] * M)
                for j in range(M):
                    assert torch.equal(bits(res[f"out{j}"][:-1]), bits(prev if val else res["h"][:-1])), f"mu = {val}: out{j}"
    for key in got:
        CHECKS.act(be, torch.cat(got[key]), torch.cat(want[key]), f"ln_mix/C{C} {key}", guard=False)


@pytest.mark.parametrize("backend,C", _params([2048, 2056, 8192]))
def test_ln_mix_row_edges(backend, be, C):
    g = be.gen(C + 2)
    rows = edge_rows(be, g, C)
    B = len(rows)
    x, prev = torch.stack([r for _, r, _ in rows]), rnd(be, g, B, C)
    lw, lb = ln_params(be, g, C)
    mus = [unif(be, g, C) for _ in range(2)]
    res = run_ln_mix(be, B, C, x, lw, lb, prev, mus)
    h = ref_ln(O64, x, lw, lb)
    for b, (name, _, cols) in enumerate(rows):
        CHECKS.act(be, res["h"][b, cols], h[b, cols], f"ln_mix/edges/C{C}/{name} h", guard=False)
        for j, mu in enumerate(mus):
            CHECKS.act(be, res[f"out{j}"][b, cols], (h + (prev.double() - h) * mu.double())[b, cols], f"ln_mix/edges/C{C}/{name} out{j}", guard=False)
        if name == "const":
            assert torch.equal(bits(res["h"][b]), bits(lb)), "zero variance: h is ln_b"


# ------------------------------------------------------------------------------------------------ tmix_head
HEAD_ARGT = [I, I] + [VP] * 7 + [VP] * 8 + [F32] + [VP] * 4


def head_inputs(be, g, B, H, D, later):
    C, nk = H * 64, 4 if later else 3
    p = dict(B=B, H=H, D=D[:nk])
    p["r"], p["k"], p["v"] = [rnd(be, g, B, C, scale=0.5) for _ in range(3)]
    p["vf"] = rnd(be, g, B, C, scale=0.5) if later else None
    hid = [rnd(be, g, B, d) for d in D[:nk]]
    hid[0], hid[2] = torch.tanh(hid[0].float()).bfloat16(), torch.sigmoid(hid[2].float()).bfloat16()
    p["hid"], p["W2t"] = hid, [rnd(be, g, C, d, scale=d ** -0.5) for d in D[:nk]]
    p["w0"], p["a0"] = rnd(be, g, C, shift=-0.5), rnd(be, g, C, scale=0.5)
    p["v0"] = rnd(be, g, C, scale=0.5, shift=1.0) if later else None
    p["k_k"], p["k_a"], p["r_k"] = rnd(be, g, C, scale=0.1, shift=0.85), rnd(be, g, C, scale=0.1, shift=1.0), rnd(be, g, C, scale=0.3)
    p["ln_w"], p["ln_b"] = rnd(be, g, C, scale=0.2, shift=1.0), rnd(be, g, C, scale=0.1)
    p["S"] = torch.randn(B, H, 64, 64, generator=g, device=be.dev) * 0.1
    return p


def run_head(be, p, carry=None):
    B, H = p["B"], p["H"]
    state = torch.full((B * H + 1, 64, 64), float("nan"), dtype=torch.float32, device=be.dev)      # in place; the last tile is the guard
    state[:-1] = p["S"].view(B * H, 64, 64)
    out = nan_rows(be, B, H * 64)
    src, dst = carry if carry is not None else (None, None)
    be.call("vrwkv_decode_tmix_head_bf16", HEAD_ARGT, B, H, P(p["r"]), P(p["k"]), P(p["v"]), P(p["vf"]), arr(p["hid"] + [None] * (4 - len(p["hid"]))),
            arr(p["W2t"] + [None] * (4 - len(p["W2t"]))), ints(list(p["D"]) + [0] * (4 - len(p["D"]))), P(p["w0"]), P(p["a0"]), P(p["v0"]),
            P(p["k_k"]), P(p["k_a"]), P(p["r_k"]), P(p["ln_w"]), P(p["ln_b"]), EPS_GN, P(state), P(out), P(src), P(dst))
    res = {"out": out, "state": state}
    written(res, None, 0)
    return res


def head_ref(o, p):
    out, S = ref_tmix(o, p["B"], p["H"], p["r"], p["k"], p["v"], p["vf"], p["hid"], p["W2t"], p["w0"], p["a0"], p["v0"], p["k_k"], p["k_a"],
                      p["r_k"], p["ln_w"], p["ln_b"], p["S"])
    return {"tmix_out": out, "tmix_state": S}


@pytest.mark.parametrize("backend,B,H,dk,layer", _params([(B, H, dk, layer) for B, H in HEAD_BH for dk in HEAD_D for layer in ("first", "later")]))
def test_tmix_head(backend, be, B, H, dk, layer):
    """Layer 0 (no value residual: v_first, v0, hid[3], W2t[3] NULL) and a later layer; with and without the carry side job.  Edges:
    lo_w + w0 at +-100; with more than one head, one head with k = 0 (the 1e-12 branch of the normalisation) and one with k = 0 and a
    zero state (y = 0: zero variance in the GroupNorm, out = ln_b * gate)."""
    later = layer == "later"
    g = be.gen(1000 * B + 10 * H + HEAD_D[dk][0] + later)
    p = head_inputs(be, g, B, H, HEAD_D[dk], later)
    C = H * 64
    p["w0"][3], p["w0"][C - 2] = 100.0, -100.0
    if B * H > 1:
        p["k"].view(B, H, 64)[0, 0] = 0
        p["k"].view(B, H, 64)[B - 1, H - 1] = 0
        p["S"][B - 1, H - 1] = 0
    tag = f"tmix_head/B{B}H{H}-{dk}-{layer}"
    res = run_head(be, p)
    same_bits(res, run_head(be, p))
    src = rnd(be, g, B + 1, C)
    dst = nan_rows(be, B, C)
    same_bits(res, run_head(be, p, carry=(src, dst)))
    assert torch.equal(bits(dst[:-1]), bits(src[:-1])) and bool(torch.isnan(dst[-1].float()).all()), "carry side job"
    ref = head_ref(O64, p)
    chain(be, "tmix_out", res["out"][:-1], ref["tmix_out"], f"{tag} out")
    chain(be, "tmix_state", res["state"][:-1].view(B, H, 64, 64), ref["tmix_state"], f"{tag} state")
    group_bias(res["out"][:-1], ref["tmix_out"], f"{tag} out")
    if be.name == "emu":
        floors(tag, lambda o: head_ref(o, p), ["tmix_out", "tmix_state"])
    if B * H > 1:
        gate = rb64(p["hid"][2][B - 1].double() @ p["W2t"][2][(H - 1) * 64:].double().t())
        want = p["ln_b"][(H - 1) * 64:].double() * gate
        assert torch.equal(res["out"][B - 1, (H - 1) * 64:].float(), want.float().bfloat16().float()), "y = 0: out = ln_b * gate"
        assert not bool(res["state"][B * H - 1].any()), "zero state, zero k: the state stays zero"
        # head (0, 0) has k = 0 and a state: S' = S diag(decay) exactly, so every column shows its decay exp(-exp(w_raw)) to fp32
        # accuracy (1-ulp exp twice and one product: < 5e-7).  A tie in lo_w or w_raw moves one column by a bf16 step of w_raw (up to
        # 7e-4); a w_raw that is not rounded where the reference rounds it moves nearly all of them.
        err = ((res["state"][0].double() - ref["tmix_state"][0, 0]).abs() / ref["tmix_state"][0, 0].abs().clamp_min(1e-30)).amax(dim=0)
        assert float((err > 2e-6).float().mean()) < 0.1, f"{tag}: decay of head (0, 0) off in {int((err > 2e-6).sum())} of 64 columns"


# ------------------------------------------------------------------------------------------------ wkv7_step
@pytest.mark.parametrize("backend", _params([()]))
def test_wkv7_step_decay_limits(backend, be):
    """w_raw in {-40, +10}: exp(-exp(w_raw)) is exactly 1 or 0 -- a column keeps its state or forgets it."""
    B, H = 3, 3
    g = be.gen(9)
    q, k, v = [rnd(be, g, B, H, 64, scale=0.5) for _ in range(3)]
    kk = torch.nn.functional.normalize(torch.randn(B, H, 64, generator=g, device=be.dev), dim=-1)
    z, a = (-kk).bfloat16(), (kk * torch.rand(B, H, 64, generator=g, device=be.dev)).bfloat16()
    w = torch.where(torch.rand(B, H, 64, generator=g, device=be.dev) < 0.5, -40.0, 10.0).bfloat16()
    S0 = torch.randn(B, H, 64, 64, generator=g, device=be.dev) * 0.3

    def run():
        state = torch.full((B * H + 1, 64, 64), float("nan"), dtype=torch.float32, device=be.dev)
        state[:-1] = S0.view(B * H, 64, 64)
        y = nan_rows(be, B * H, 64)
        be.call("vrwkv_wkv7_step_bf16", [I, I] + [VP] * 8, B, H, P(w), P(q), P(k), P(v), P(z), P(a), P(state), P(y))
        written({"y": y, "state": state}, None, 0)
        return {"y": y, "state": state}

    res = run()
    same_bits(res, run())
    y_ref, s_ref = wkv7_naive(*[t.double().unsqueeze(1) for t in (w, q, k, v, z, a)], state0=S0.double())
    CHECKS.act(be, res["y"], y_ref[:, 0].reshape(B * H, 64), "wkv7_step y")
    got = res["state"][:-1].view(B, H, 64, 64)
    assert rel_rms(got, s_ref) < 2e-6          # fp32 state (tests/test_stateful_gpu.py)
    decay = torch.exp(-torch.exp(w.double()))
    assert bool(((decay == 0) | (decay == 1)).all()) and bool((decay == 0).any()) and bool((decay == 1).any())


# ------------------------------------------------------------------------------------------------ argument rejections
def _nan_like(be, *shape):
    return torch.full(shape, float("nan"), dtype=torch.bfloat16, device=be.dev)


def _untouched(*bufs):
    for b in bufs:
        assert bool(torch.isnan(b.float()).all()), "a rejected call wrote to an output"


def _pad(t, n=8):
    """The tensor's elements followed by n spare ones: a pointer 2 bytes into it still has the whole tensor in front of it."""
    return torch.cat([t.reshape(-1), torch.zeros(n, dtype=t.dtype, device=t.device)])


# The refusal tables below are read off the entries as they stand: every count at 0 and one past its cap, every width just off its
# modulus, every pointer NULL in turn, every pointer the entry checks for alignment 2 bytes off (fp32: 4), and for the pointers it does
# not check (they are read and written by element) one accepted call with all of them 2 bytes off.  The order of the checks is part of
# the table: the cases marked "two faults" expect the code of the check that comes first.  Every buffer has spare rows: no case depends
# on being refused to stay in bounds.
@pytest.mark.parametrize("backend", _params([()]))
def test_rejects_gemv(backend, be):
    g = be.gen(3)
    B, N, K = 2, 9, 64
    W, x, y, res = rnd(be, g, N + 1, K), rnd(be, g, 5 + 1, K), _nan_like(be, 5 + 1, N), rnd(be, g, 5 + 1, N)
    src, dst = rnd(be, g, 64), _nan_like(be, 64)
    T = [I, I] + [VP] * 7

    def go(n=1, B=B, W=W.data_ptr(), x=x.data_ptr(), y=y.data_ptr(), res=None, N=N, K=K, null=(), copy=None):
        m = max(n, 1)
        a = dict(W=arr([W] * m), x=arr([x] * m), res=arr([res] * m) if res is not None else None, y=arr([y] * m), N=ints([N] * m), K=ints([K] * m),
                 act=ints([0] * m))
        args = [n, B] + [None if k in null else a[k] for k in ("W", "x", "res", "y", "N", "K", "act")]
        if copy is None:
            return rc_of(be, "vrwkv_gemv_multi_bf16", T, *args)
        return rc_of(be, "vrwkv_gemv_multi_copy_bf16", T + [VP, VP, L], *args, VP(copy[0]), VP(copy[1]), copy[2])

    def cp(s, d, elems, **kw):
        return go(copy=(s, d, elems), **kw)

    sp, dp = src.data_ptr(), dst.data_ptr()
    for both in (go, lambda **kw: cp(sp, dp, 8, **kw)):          # the copy entry runs the same checks on its jobs
        assert both(n=0) == EINVAL and both(n=9) == EINVAL
        assert both(B=0) == EINVAL and both(B=5) == EINVAL
        for name in ("W", "x", "y", "N", "K", "act"):
            assert both(null=(name,)) == EINVAL, name
        assert both(W=None) == ESHAPE and both(x=None) == ESHAPE and both(y=None) == ESHAPE        # a NULL job pointer answers like a bad N or K
        assert both(K=60) == ESHAPE and both(K=0) == ESHAPE and both(N=0) == ESHAPE
        assert both(W=W.data_ptr() + 2) == EALIGN and both(x=x.data_ptr() + 2) == EALIGN
        # two faults
        assert both(B=5, K=60) == EINVAL and both(n=0, null=("W",)) == EINVAL
        assert both(W=None, x=x.data_ptr() + 2) == ESHAPE and both(K=60, W=W.data_ptr() + 2) == ESHAPE
    assert cp(sp, dp, 12) == ESHAPE and cp(sp, dp, -8) == EINVAL
    assert cp(None, dp, 8) == EINVAL and cp(sp, None, 8) == EINVAL
    assert cp(sp + 2, dp, 8) == EALIGN and cp(sp, dp + 2, 8) == EALIGN
    assert cp(sp + 2, None, 0) == EALIGN                                   # the copy pointers are checked whatever copy_elems is
    # two faults: the copy side job is checked after the counts and before the jobs
    assert cp(sp, dp, 12, n=0) == EINVAL and cp(None, dp, 8, K=60) == EINVAL
    assert cp(sp + 2, dp, 12) == ESHAPE and cp(sp, dp, 12, K=60) == ESHAPE and cp(sp, dp + 2, 8, W=None) == EALIGN
    _untouched(y, dst)
    y2 = _nan_like(be, 5 + 1, N)
    assert go(y=y2.data_ptr() + 2, res=res.data_ptr() + 2) == 0            # y and res are not checked for alignment: element accesses
    assert bool(torch.isfinite(y2.reshape(-1)[1:1 + B * N].float()).all()) and bool(torch.isnan(y2.reshape(-1)[1 + B * N:].float()).all())
    _untouched(y, dst)
    assert go() == 0                            # the same arguments without the fault are accepted
    assert bool(torch.isfinite(y[:B].float()).all())


@pytest.mark.parametrize("backend", _params([()]))
def test_rejects_fold(backend, be):
    g = be.gen(4)
    B, N = 2, 9
    y, h = _nan_like(be, 5 + 1, N), _nan_like(be, 5 + 1, 4104)
    T = [I, I, I, VP, VP, VP, VP, F32] + [VP] * 6

    def go(K=512, n=1, B=B, N=N, mu=0, null=(), off=(), y=y, h=h):
        Kt = max(K, 8)
        t = dict(W=rnd(be, g, N + 1, Kt), x=rnd(be, g, 5 + 1, Kt), ln_w=rnd(be, g, Kt + 8), ln_b=rnd(be, g, Kt + 8), x_prev=rnd(be, g, 5 + 1, Kt),
                 mu=rnd(be, g, Kt + 8), h=h, y=y)
        ad = {k: (0 if k in null else v.data_ptr() + (2 if k in off else 0)) for k, v in t.items()}
        m = max(n, 1)
        ad["mu"] = 0 if mu is None else ad["mu"] + mu
        arrays = dict(Wa=arr([ad["W"]] * m), mua=arr([ad["mu"]] * m), ya=arr([ad["y"]] * m), Na=ints([N] * m), acta=ints([0] * m))
        arrays = {k: (None if k in null else v) for k, v in arrays.items()}
        return rc_of(be, "vrwkv_gemv_ln_multi_bf16", T, n, B, K, arrays["Wa"], VP(ad["x"]), VP(ad["ln_w"]), VP(ad["ln_b"]), EPS_LN, VP(ad["x_prev"]),
                     arrays["mua"], VP(ad["h"]), arrays["ya"], arrays["Na"], arrays["acta"])

    assert go(K=504) == ESHAPE and go(K=4104) == ESHAPE and go(K=516) == ESHAPE and go(K=0) == ESHAPE and go(N=0) == ESHAPE
    assert go(mu=None) == EINVAL and go(mu=2) == EALIGN
    assert go(n=0) == EINVAL and go(n=9) == EINVAL and go(B=0) == EINVAL and go(B=5) == EINVAL
    for name in ("x", "ln_w", "ln_b", "x_prev", "h", "Wa", "mua", "ya", "Na", "acta"):
        assert go(null=(name,)) == EINVAL, name
    assert go(null=("W",)) == ESHAPE and go(null=("y",)) == ESHAPE
    for name in ("W", "x", "ln_w", "ln_b", "x_prev", "h"):
        assert go(off=(name,)) == EALIGN, name
    # two faults: the entry's own pointers come before the launcher's counts and jobs
    assert go(off=("ln_w",), B=0) == EALIGN and go(n=0, off=("ln_w",)) == EINVAL and go(null=("x",), off=("h",)) == EINVAL
    assert go(K=504, mu=None) == ESHAPE and go(null=("W",), off=("x",)) == ESHAPE and go(K=4104, mu=2) == ESHAPE
    _untouched(y, h)
    y2, h2 = _nan_like(be, 5 + 1, N), _nan_like(be, 5 + 1, 512)
    assert go(off=("y",), y=y2, h=h2) == 0                                 # y is not checked for alignment: element stores
    assert bool(torch.isfinite(y2.reshape(-1)[1:1 + B * N].float()).all()) and bool(torch.isnan(y2.reshape(-1)[1 + B * N:].float()).all())
    _untouched(y, h)
    assert go() == 0
    assert bool(torch.isfinite(y[:B].float()).all()) and bool(torch.isfinite(h.reshape(-1)[:B * 512].float()).all())


@pytest.mark.parametrize("backend", _params([()]))
def test_rejects_ln_mix(backend, be):
    g = be.gen(5)
    B = 2
    outs = [_nan_like(be, B, 8200) for _ in range(7)]
    T = [I, I, I, VP, VP, VP, F32, VP, VP, VP]

    def go(B=B, C=64, M=2, null=(), off=(), mu_at=None, out_at=None):
        Ct = max(C, 8)
        t = dict(x=rnd(be, g, 2 + 1, Ct), ln_w=rnd(be, g, Ct + 8), ln_b=rnd(be, g, Ct + 8), x_prev=rnd(be, g, 2 + 1, Ct))
        keep = t["x_prev"].clone()
        ad = {k: VP(0 if k in null else v.data_ptr() + (2 if k in off else 0)) for k, v in t.items()}
        mus, os_ = [rnd(be, g, Ct + 8).data_ptr() for _ in range(7)], [o.data_ptr() for o in outs]
        if mu_at is not None:
            mus[mu_at[0]] = mus[mu_at[0]] + 2 if mu_at[1] else 0
        if out_at is not None:
            os_[out_at[0]] = os_[out_at[0]] + 2 if out_at[1] else 0
        rc = rc_of(be, "vrwkv_decode_ln_mix_bf16", T, B, C, M, ad["x"], ad["ln_w"], ad["ln_b"], EPS_LN, ad["x_prev"],
                   None if "mu" in null else arr(mus), None if "out" in null else arr(os_))
        assert rc == 0 or torch.equal(bits(t["x_prev"]), bits(keep)), "a rejected call replaced the carried row"
        return rc

    assert go(C=12) == ESHAPE and go(C=8200) == ESHAPE and go(C=0) == ESHAPE
    assert go(M=7) == EINVAL and go(M=0) == EINVAL and go(B=0) == EINVAL
    for name in ("x", "ln_w", "ln_b", "x_prev", "mu", "out"):
        assert go(null=(name,)) == EINVAL, name
    assert go(mu_at=(1, 0)) == EINVAL and go(out_at=(0, 0)) == EINVAL
    for name in ("x", "ln_w", "ln_b", "x_prev"):
        assert go(off=(name,)) == EALIGN, name
    assert go(mu_at=(0, 2)) == EALIGN and go(out_at=(1, 2)) == EALIGN
    # two faults
    assert go(M=7, C=12) == EINVAL and go(C=12, off=("x",)) == ESHAPE and go(mu_at=(1, 0), off=("x",)) == EINVAL
    _untouched(*outs)
    assert go(mu_at=(2, 0)) == 0 and go(out_at=(2, 2)) == 0                 # past M: not looked at
    assert go() == 0


@pytest.mark.parametrize("backend", _params([()]))
def test_rejects_tmix_head(backend, be):
    g = be.gen(6)
    B, H = 2, 2
    C = H * 64
    p = head_inputs(be, g, B + 1, H, HEAD_D["D32"], later=True)
    names = ("r", "k", "v", "vf", "w0", "a0", "v0", "k_k", "k_a", "r_k", "ln_w", "ln_b")
    t = {n: _pad(p[n]) for n in names}
    t["hid"], t["W2t"] = [_pad(h) for h in p["hid"]], [_pad(w) for w in p["W2t"]]
    t["src"], t["out"], t["dst"] = rnd(be, g, (B + 1) * C + 8), _nan_like(be, (B + 1) * C + 8), _nan_like(be, (B + 1) * C + 8)
    t["state"] = torch.full(((B + 1) * H * 4096 + 4,), float("nan"), dtype=torch.float32, device=be.dev)

    def go(B=B, H=H, D=p["D"], null=(), off=(), carry=False, hid_at=None, w2_at=None, t=t):
        def ad(n):
            return VP(0 if n in null else t[n].data_ptr() + ((4 if n == "state" else 2) if n in off else 0))
        hid, w2 = [h.data_ptr() for h in t["hid"]], [w.data_ptr() for w in t["W2t"]]
        if hid_at is not None:
            hid[hid_at[0]] = hid[hid_at[0]] + 2 if hid_at[1] else 0
        if w2_at is not None:
            w2[w2_at[0]] = w2[w2_at[0]] + 2 if w2_at[1] else 0
        src = ad("src") if carry in (True, "src") else None
        dst = ad("dst") if carry in (True, "dst") else None
        return rc_of(be, "vrwkv_decode_tmix_head_bf16", HEAD_ARGT, B, H, ad("r"), ad("k"), ad("v"), ad("vf"), None if "hid" in null else arr(hid),
                     None if "W2t" in null else arr(w2), None if "D" in null else ints(list(D)), ad("w0"), ad("a0"), ad("v0"), ad("k_k"), ad("k_a"),
                     ad("r_k"), ad("ln_w"), ad("ln_b"), EPS_GN, ad("state"), ad("out"), src, dst)

    assert go(B=0) == EINVAL and go(H=0) == EINVAL
    assert go(D=(48, 32, 32, 32)) == ESHAPE and go(D=(32, 32, 0, 32)) == ESHAPE and go(D=(32, 32, 32, 16)) == ESHAPE
    assert go(carry="src") == EINVAL and go(carry="dst") == EINVAL
    for name in ("r", "k", "v", "hid", "W2t", "D", "w0", "a0", "k_k", "k_a", "r_k", "ln_w", "ln_b", "state", "out"):
        assert go(null=(name,)) == EINVAL, name
    assert go(null=("v0",)) == EINVAL                                      # a value residual (v_first) needs v0
    assert go(hid_at=(1, 0)) == EINVAL and go(w2_at=(3, 0)) == EINVAL
    assert go(off=("state",)) == EALIGN and go(hid_at=(0, 2)) == EALIGN and go(w2_at=(2, 2)) == EALIGN
    # two faults: the state's alignment comes before the LoRA loop, which takes NULL, width, alignment factor by factor
    assert go(D=(48, 32, 32, 32), off=("state",)) == EALIGN and go(null=("r",), off=("state",)) == EINVAL and go(B=0, carry="src") == EINVAL
    assert go(D=(48, 32, 32, 32), hid_at=(1, 0)) == ESHAPE and go(D=(48, 32, 32, 32), hid_at=(0, 0)) == EINVAL
    assert go(D=(32, 48, 32, 32), hid_at=(0, 2)) == EALIGN
    _untouched(t["out"], t["dst"], t["state"])
    # what the entry reads and writes by element is not checked for alignment: all of it 2 bytes off in one accepted call; layer 0
    # (v_first NULL) takes neither v0 nor the fourth LoRA pair
    t2 = dict(t, out=_nan_like(be, (B + 1) * C + 8), dst=_nan_like(be, (B + 1) * C + 8), state=torch.zeros_like(t["state"]))
    assert go(off=names + ("out", "src", "dst"), carry=True, t=t2) == 0
    assert bool(torch.isfinite(t2["out"][1:1 + B * C].float()).all()) and bool(torch.isnan(t2["out"][1 + B * C:].float()).all())
    assert torch.equal(bits(t2["dst"][1:1 + B * C]), bits(t2["src"][1:1 + B * C])) and bool(torch.isnan(t2["dst"][1 + B * C:].float()).all())
    t2["state"].zero_()
    assert go(null=("vf", "v0"), hid_at=(3, 0), w2_at=(3, 0), D=(32, 32, 32, 0), t=t2) == 0
    _untouched(t["out"], t["dst"], t["state"])


@pytest.mark.parametrize("backend", _params([()]))
def test_rejects_wkv7_step(backend, be):
    g = be.gen(7)
    names = ("w", "q", "k", "v", "z", "a")
    t = {n: rnd(be, g, 2 * 64 + 8, scale=0.1) for n in names}
    t["y"] = _nan_like(be, 2 * 64 + 8)
    t["state"] = torch.full((2 * 4096 + 4,), float("nan"), dtype=torch.float32, device=be.dev)

    def go(B=1, H=1, null=(), off=(), t=t):
        ad = [VP(0 if n in null else t[n].data_ptr() + ((4 if n == "state" else 2) if n in off else 0)) for n in names + ("state", "y")]
        return rc_of(be, "vrwkv_wkv7_step_bf16", [I, I] + [VP] * 8, B, H, *ad)

    assert go(B=0) == EINVAL and go(H=0) == EINVAL                          # no cap on either: one workgroup per (b, h)
    for name in names + ("state", "y"):
        assert go(null=(name,)) == EINVAL, name
    assert go(off=("state",)) == EALIGN
    assert go(null=("w",), off=("state",)) == EINVAL and go(B=0, off=("state",)) == EINVAL          # two faults
    _untouched(t["y"], t["state"])
    t2 = dict(t, y=_nan_like(be, 2 * 64 + 8), state=torch.zeros_like(t["state"]))
    assert go(off=names + ("y",), t=t2) == 0                                # the vectors are read and written by element: not checked
    assert bool(torch.isfinite(t2["y"][1:65].float()).all()) and bool(torch.isnan(t2["y"][65:].float()).all())
    assert go(B=2, t=t2) == 0
    _untouched(t["y"], t["state"])


# ------------------------------------------------------------------------------------------------ entries that forward to one launcher
@pytest.mark.parametrize("backend", _params([()]))
def test_gemv_entries_agree(backend, be):
    """vrwkv_gemv_multi_bf16, the copy entry with copy_elems = 0 and the gated entry with a gate of ones and no copy: a product times 1.0
    is exact, so the three give the same bits.  One launch of three jobs on the three K paths at their edges: K = 64 (short rows), 512
    (exactly GV_LONG_KCHUNKS chunks), 2080 (the smallest K > 2048 with K % 32 == 0); N = 9 leaves the last workgroup partial (32 and 8
    rows per workgroup), N = 3 the split-K tail (2 rows)."""
    B = 2
    jobs = gemv_jobs(be, be.gen(11), B, [(9, 64), (9, 512), (3, 2080)], rot=3)       # activations 3, 0, 1; residuals on the first and the last
    plain = run_gemv(be, B, jobs)
    copy0 = run_gemv(be, B, jobs, copy=(None, None, 0))
    gated = [nan_rows(be, B, j["W"].shape[0]) for j in jobs]
    ones = [torch.ones(B, j["W"].shape[0], dtype=torch.bfloat16, device=be.dev) for j in jobs]
    be.call("vrwkv_gemv_gated_copy_bf16", [I, I] + [VP] * 10 + [L], len(jobs), B, arr([j["W"] for j in jobs]), arr([j["x"] for j in jobs]),
            arr([j["res"] for j in jobs]), arr(ones), arr(gated), ints([j["W"].shape[0] for j in jobs]), ints([j["W"].shape[1] for j in jobs]),
            ints([j["act"] for j in jobs]), None, None, 0)
    written({f"y{j}": y for j, y in enumerate(gated)}, None, 0)
    assert any(j["res"] is not None for j in jobs) and any(j["res"] is None for j in jobs)
    same_bits(dict(enumerate(copy0)), dict(enumerate(plain)))
    same_bits(dict(enumerate(gated)), dict(enumerate(plain)))
    check_gemv(be, [(B, jobs, plain)], "gemv/entries")


def test_fold_cases_reach_every_instantiation():
    """gemv_ln_kernel<CH, BB>: CH = 2 chunks per thread for K > 2048, BB = 1, 2 or 4 batch rows compiled in (3 rides on 4).  test_fold's
    K x B grid reaches all six, and B = 3 on both sides of 2048."""
    inst = lambda K, B: (2 if K > 2048 else 1, 1 if B == 1 else 2 if B == 2 else 4)
    grid = [(K, B) for K, _ in FOLD_K for B in (1, 2, 3, 4)]
    assert {inst(K, B) for K, B in grid} == {(ch, bb) for ch in (1, 2) for bb in (1, 2, 4)}
    assert {inst(K, 3) for K, B in grid if B == 3} == {(1, 4), (2, 4)}
    assert all(512 <= K <= 4096 and K % 8 == 0 for K, _ in grid)
