"""The LayerNorm half of the per-layer glue -- csrc/ln_fused.hip with csrc/ln_kernels.h (add + LayerNorm, the same fused with the
token shift and its lerps, the scatter / gather and the scaled forms) and the M = 6 token-shift backward that recomputes the LayerNorm
output (vrwkv_mix_bwd_ln{,_packed,_carry}_bf16 of csrc/tmix_fused.hip) -- at the shapes where the launch code and the kernels change
their path, through the C ABI, on two backends with the same test bodies: the host lockstep emulator (tests/emu/emu_ln_fused.cpp
compiles ln_fused.hip whole: CPU tensors, no marker) and the product library (CUDA tensors, `gpu` marker).

What picks the path (see SHAPES).  Forward: one workgroup per row (add_ln, scatter), ranges of 4 rows with the predecessor row
recomputed (ln_mix_fwd).  Backward: one workgroup per row until ntok passes the cap, then contiguous ranges lo = ntok g / G,
hi = ntok (g + 1) / G with the next row prefetched -- G = min(ntok, 1024) for add_ln_bwd / ln_gather_bwd, min(ntok, 768) for
ln_mix_bwd (ws split at G 2 C), min(ceil(ntok / 16), 1024) for mix_bwd_ln; ln_mix_bwd and mix_bwd_ln read the look-ahead row `hi`
unless it opens a sample.  More than 64 partial rows give ln_colsum / colsum a second trip.  Row width: C / 8 threads rounded up to
a wave (a partial wave for C = 192, 576, 2112, 4160), ln_mix_bwd compiled for 256 / 512 / 1024 threads, mix_bwd_ln's channel loop
(C > 2048).

Reference: torch autograd in fp64 on the same bf16 inputs (ref_ln, ref_mix_chain below), on the backend's device, LayerNorm spelled
out in elementary ops (see test_glue_shapes.py on the fused norm backward of this torch build).  It models the roundings the kernel
headers document and nothing else: xn = bf16(x + delta [dscale]) and y = bf16(LN(xn)) are value-rounded with a straight-through
gradient; the gradient that arrives at y (all lerps, and dy_last at a sample's last row) is rounded to bf16 once (RoundGrad: the
documented dyl = bf16(A + Bv), the bf16 dx that mix_bwd_ln hands to add_ln_bwd); y_prev is an fp64 leaf whose gradient is dy_prev.
One more thing had to be modelled (near_tie): where the fp64 value of y, or of the summed gradient at y, lies on a bf16 rounding
boundary, the fp32 kernel and the fp64 reference may round to different neighbours (1e-5 .. 1e-4 of the elements do).  The flip of y
and of dy (M = 6) itself is counted under point 1, against the pure fp64 rounding.  But everything downstream sees it in full:
dmu_c = sum_n d[n, c] (y[n-1, c] - y[n, c]) moves by ulp_bf16(y) |d| -- 5e-4 of rms(dmu) at 19 tokens, by sqrt(ntok) less at more
(measured: ln_mix lb512_first carry:l, channel 917, one flipped y of 40 128), as much as the dropped partial row that PERR is there to
show.  So at those elements, and only there, the reference continues with the neighbour the kernels chose: y as vrwkv_add_ln_fwd_bf16
returns it for the same inputs (the fused forward saves the same xn, mean and rstd bit for bit -- asserted -- and the shift check
below ties its outputs to that y), the gradient as mix_bwd_ln returns it (M = 6; ln_mix_bwd keeps it in registers, and its
d (1 - mu) + d' mu is exact in fp32 but for the last addition).  "On a boundary" is: the kernel's value is no further from the fp64
value v than bf16(v) is, plus a slack of min(SLACK (1 + |v|), ulp_bf16(v) / 4), SLACK = 2^-17 = 64 fp32 ulps of 1.  The first term is
what fp32 arithmetic on operands of that size can move v by; the second caps it for small v, so that whatever |v|, only one of the two
bf16 values around v can be taken over, and only where v is within ulp_bf16(v) / 8 of their midpoint.  Any other kernel value is left to
fail against bf16(v).  What follows from y and dy -- out_j, y_last, dx, dw, db, dmu, dy_prev -- is compared with this kernel-informed
reference, which differs from the pure one at those boundary elements alone.
Every case asserts
  1. activations and activation gradients: tests.parity.bf16_close against the reference rounded once, tol 1e-3, flips <= FLIP;
  2. dwb, dmu and dy_prev in fp32, per vector: max_c |got_c - ref_c| / rms_c(ref) <= PERR, and tests.parity.group_bias;
  3. mean and rstd against fp64 under the same PERR: |mean - ref| / sqrt(ref^2 + var + eps) and |rstd - ref| / ref, worst row;
  4. outputs, parameter gradients and ws are NaN before the call, every buffer ends in a guard row and ws in C guard floats after
     vrwkv_*_ws_floats: results finite, guards untouched;
  5. a second call is bit-identical.
Edges that ride along: an all-zero row and a row that is constant over its channels (zero variance, rstd = 1 / sqrt(eps)); the exact
shift indexing: ln_mix_fwd with mu = 1 gives, bit for bit, the y that add_ln_fwd gives for the row before, zeros at every sample or
segment start, and the y_prev row where one is carried in.  (fma(yp - y, 1, y) rounds to the bf16 value yp whenever |y| < 2^15 |yp|;
that check runs with w = 1/4, b = 3, which keeps every y in about [1.5, 4.5].)  For the capped shapes the case asserts, from the
kernel's own range formula, that sample starts (and, packed, the drawn segment starts) fall where PLAIN_STARTS says: at a range's
first row, strictly inside a range, at a look-ahead row hi < ntok.

  id             (B, T, C)        what it reaches
  one_token      (1, 1, 64)       one token, one workgroup per row
  t1_samples     (3, 1, 64)       T = 1: every row opens a sample; one ln_mix_fwd range of 3 rows
  ragged_fwd     (1, 17, 64)      ln_mix_fwd ranges of 3-4 rows (ntok % 4 != 0) with the predecessor recomputed at lo - 1
  caps           (3, 375, 64)     both backward caps (1024 and 768: ranges of 1-2 rows), colsum's second trip for mix_bwd_ln (G = 71);
                                  sample starts at a range start / hi (ln_mix_fwd, ln_mix_bwd) and inside a range (mix_bwd_ln)
  caps_b5        (5, 225, 64)     ln_mix_bwd under the 768 cap: a sample start on the second row of a two-row range
  caps_t16       (3, 368, 64)     mix_bwd_ln (G = 69, ranges of 16): sample starts at a range start / hi
  deep           (3, 4115, 64)    12-17 rows per workgroup under both caps: the next-row prefetch in steady state
  mix_cap        (3, 5471, 64)    mix_bwd_ln's own cap, G = 1024 of 1026 (the emulator runs only mix_bwd_ln here)
  partial_wave   (1, 37, 192)     24 of 64 lanes
  one_wave       (1, 37, 512)     exactly one wave
  wave2_8        (1, 37, 576)     a second wave with 8 active lanes
  lb256_full     (1, 37, 2048)    ln_mix_bwd <256> full
  lb512_first    (1, 37, 2112)    <512>: 264 lanes in a 320 block; mix_bwd_ln's channel loop with a second trip
  lb512_full     (1, 37, 4096)
  lb1024_first   (1, 37, 4160)    <1024>: 520 lanes in a 576 block
  lb1024_full    (1, 37, 8192)    the largest C ln_ok admits
  x_wide_deep    (3, 4115, 2112)  GPU only: wide rows under the caps, 12-17 rows per workgroup
  x_wide_1024    (3, 1500, 4160)  GPU only: the <1024> kernels under the caps
The emulator walks rows of C >= 2048 with 19 tokens instead of 37 (about 1 ms per row and kernel with a barrier in it).  At `deep` and
`mix_cap` (12 345 and 16 413 rows) a case with one backward kernel alone takes it 14 to 15 s, so there it runs the backward kernels alone -- add_ln_bwd
and ln_mix_bwd once, mix_bwd_ln twice and without add_ln_bwd behind it -- on a forward computed by host_fwd, and no add_ln_scaled_fwd;
the forward kernels take one to four rows per workgroup at any ntok, so what the depth adds lies in the backward.  Not asserted on the
emulator at those two shapes: point 5 for add_ln_bwd and ln_mix_bwd (M = 1); of point 1 xn, y, out_j and y_last as kernel output, and
for mix_bwd_ln (M = 6) the dx of the chain; of point 2 the chain's dw and db (M = 6); point 3; the shift check.  Points 1, 2 and 4 hold
there for what the backward kernels write (dx, dwb, dmu, dy_prev for M = 1; dy, dmu, dy_prev for M = 6).  The MI355X backend asserts all
five points at every shape.

Bounds.  FLIP and PERR are 4 x the worst value observed over all cases of a backend (the arithmetic is deterministic; the margin is
for other seeds and other boxes) and have to stay at or below the project's 0.01 (FLIP_Y of test_wkv7_gpu.py) and 1e-4 (parameter
gradients in test_emulated_tmix.py).  VRWKV_TEST_NOTES=1 prints every figure and the running worst.
Observed (worst case over the module, the case that gave it):
  emulator (host libm):  flips 2.815e-04 (mix_bwd_ln partial_wave plain+dup3 dx: two elements of 7104), parameter gradients and
                         statistics 8.134e-07 (ln_mix lb512_full plain+dres dw)  ->  FLIP 1.2e-3, PERR 3.3e-6
  MI355X:                flips 9.191e-04 (ln_mix ragged_fwd packed y: one element of 1088), parameter gradients and statistics
                         9.355e-07 (mix_bwd_ln mix_cap plain+dup3 dmu2)  ->  FLIP 3.7e-3, PERR 3.8e-6
"""

import pytest
import torch

from tests.shape_checks import Checks
from tests.test_glue_shapes import Backend, F32, I, L, P, PA, VP, bits, f64, nan_rows, rnd, same_bits, unif, written

EPS = 1e-5
TOL = 1e-3
FLIP = {"emu": 1.2e-3, "hip": 3.7e-3}          # 4 x observed (module docstring)
PERR = {"emu": 3.3e-6, "hip": 3.8e-6}
SLACK = 2.0 ** -17                          # near_tie: 64 fp32 ulps of 1 + |v|, capped at ulp_bf16(v) / 4
EINVAL, ESHAPE = -1, -2

BACKENDS = ["emu", pytest.param("hip", marks=pytest.mark.gpu)]
SHAPES = [      # the table of the module docstring
    ("one_token",    1, 1,    64),
    ("t1_samples",   3, 1,    64),
    ("ragged_fwd",   1, 17,   64),
    ("caps",         3, 375,  64),
    ("caps_b5",      5, 225,  64),
    ("caps_t16",     3, 368,  64),
    ("deep",         3, 4115, 64),
    ("mix_cap",      3, 5471, 64),
    ("partial_wave", 1, 37,   192),
    ("one_wave",     1, 37,   512),
    ("wave2_8",      1, 37,   576),
    ("lb256_full",   1, 37,   2048),
    ("lb512_first",  1, 37,   2112),
    ("lb512_full",   1, 37,   4096),
    ("lb1024_first", 1, 37,   4160),
    ("lb1024_full",  1, 37,   8192),
    ("x_wide_deep",  3, 4115, 2112),
    ("x_wide_1024",  3, 1500, 4160),
]
FULL_MATRIX = ("caps", "lb512_first")
GPU_ONLY = ("x_wide_deep", "x_wide_1024")
SHIFT_ONLY = ("caps_b5", "caps_t16")       # shapes that differ from `caps` only in where the sample starts fall: the token-shift families
EMU_WIDE_T = 19
EMU_HEAVY = ("deep", "mix_cap")           # 12 345 and 16 413 rows: about 1 ms per row and kernel on the emulator
LN_BWD_GRID, LN_MIX_BWD_GRID, MIX_BWD_GRID, MIX_TPB, LN_MIX_FWD_ROWS = 1024, 768, 1024, 16, 4       # the product's values
# where the starts of the UNPACKED layout fall in each kernel's ranges (asserted: a changed cap must not silently empty a case)
PLAIN_STARTS = {
    ("caps", "ln_mix_fwd"): {"lo", "hi"}, ("caps", "ln_mix_bwd"): {"lo", "hi"}, ("caps", "mix_bwd_ln"): {"inside"},
    ("caps_b5", "ln_mix_bwd"): {"lo", "inside", "hi"},
    ("caps_t16", "mix_bwd_ln"): {"lo", "hi"},
    ("deep", "ln_mix_bwd"): {"lo", "hi"}, ("deep", "mix_bwd_ln"): {"inside"},
}
PACKED_STARTS = ("caps", "caps_b5", "caps_t16", "deep", "mix_cap", "x_wide_deep", "x_wide_1024")     # drawn marks: all three kinds, every kernel


def _cases(configs_full=None, configs_rest=None, shift=False, emu_heavy=()):
    """(backend, shape[, config]) of one test: the full option matrix at FULL_MATRIX, `configs_rest` elsewhere.  The emulator gets no GPU_ONLY shape
    and of EMU_HEAVY those in `emu_heavy` (there the test runs the backward kernels alone, see _mix_case)."""
    out = []
    for b in BACKENDS:
        name, marks = (b, ()) if isinstance(b, str) else (b.values[0], b.marks)
        for sid, _, _, _ in SHAPES:
            if name == "emu" and (sid in GPU_ONLY or (sid in EMU_HEAVY and sid not in emu_heavy)):
                continue
            if sid in SHIFT_ONLY and not shift:
                continue
            for cfg in ([None] if configs_full is None else configs_full if sid in FULL_MATRIX else configs_rest):
                vals = (name, sid) if cfg is None else (name, sid, cfg)
                out.append(pytest.param(*vals, id="-".join(vals), marks=marks))
    return out


class LnBackend(Backend):
    def shape(self, sid):
        _, B, T, C = next(s for s in SHAPES if s[0] == sid)
        if self.name == "emu" and C >= 2048:
            T = EMU_WIDE_T
        return B, T, C

    def rc(self, fn, argtypes, *args):
        f = getattr(self.lib, fn)
        f.argtypes, f.restype = argtypes + [VP], I
        return int(f(*args, self.stream))

    def ws(self, fn, *args):
        f = getattr(self.lib, fn)
        f.argtypes, f.restype = [L, I] + [I] * (len(args) - 2), L
        return int(f(*args))


@pytest.fixture
def be(request, backend):
    return LnBackend(request, backend)


# ------------------------------------------------------------------------------------------------ checks
CHECKS = Checks("ln", FLIP, PERR, TOL)
note, act, par = CHECKS.note, CHECKS.act, CHECKS.par


def stats(be, mean, rstd, ref, name):
    """The saved row statistics (ntok + guard, 1) against fp64: the mean relative to the row's rms, rstd relative to itself."""
    m, r = mean[:-1, 0].double(), rstd[:-1, 0].double()
    em = ((m - ref["mean"]).abs() / (ref["mean"].pow(2) + ref["var"] + EPS).sqrt()).max()
    er = ((r - ref["rstd"]).abs() / ref["rstd"]).max()
    for kind, e in (("mean", float(em)), ("rstd", float(er))):
        note(be, "perr", e, f"{name} {kind}")
        assert e < PERR[be.name], f"{name} {kind}: worst row off by {e:.3e} (relative)"


def nan_ws(be, floats, C):
    return torch.full((floats + C,), float("nan"), dtype=torch.float32, device=be.dev)


def edges(x, delta):
    """One all-zero row and one row that is constant over its channels (zero variance), placed in xn = x + delta."""
    ntok = x.shape[0]
    if ntok >= 3:
        x[ntok // 2] = 0.0
        x[ntok - 1] = 1.5
        if delta is not None:
            delta[ntok // 2] = 0.0
            delta[ntok - 1] = 0.0


def ranges(ntok, G):
    return [(ntok * g // G, ntok * (g + 1) // G) for g in range(G)]


def start_kinds(ntok, G, starts):
    """Where the starts (row numbers > 0) fall in the G ranges of a kernel: at a range's first row, strictly inside, at its look-ahead row."""
    s, kinds = set(int(v) for v in starts if v > 0), set()
    for lo, hi in ranges(ntok, G):
        if lo >= hi:
            continue
        if lo in s:
            kinds.add("lo")
        if any(n in s for n in range(lo + 1, hi)):
            kinds.add("inside")
        if hi < ntok and hi in s:
            kinds.add("hi")
    return kinds


def grids(ntok, M):
    g = {"ln_mix_fwd": (ntok + LN_MIX_FWD_ROWS - 1) // LN_MIX_FWD_ROWS}
    if M == 1:
        g["ln_mix_bwd"] = min(ntok, LN_MIX_BWD_GRID)
    else:
        g["mix_bwd_ln"] = min((ntok + MIX_TPB - 1) // MIX_TPB, MIX_BWD_GRID)
    return g


def draw_first(be, ntok, T, M):
    """Segment marks of a packed layout: for every kernel of the family one at a range's first row (= the look-ahead row of the range before)
    and one strictly inside a range, a one-token segment, and a few at random."""
    first = torch.zeros(ntok, dtype=torch.uint8)
    for k, G in enumerate(grids(ntok, M).values()):
        rs = [r for r in ranges(ntok, G) if r[0] < r[1]]
        at = rs[(len(rs) * (1 + k)) // 4]
        if at[0] > 0:
            first[at[0]] = 1
        deep = [r for r in rs if r[1] - r[0] >= 2]
        if deep:
            first[deep[(len(deep) * (2 + k)) // 5][0] + 1] = 1
    if ntok >= 4:
        first[ntok // 2] = 1
        first[ntok // 2 + 1] = 1
        first[torch.randint(1, ntok, (max(1, ntok // 50),), generator=torch.Generator().manual_seed(ntok))] = 1
    return first.to(be.dev)


# ------------------------------------------------------------------------------------------------ reference (fp64)
def ste(v):
    """bf16(v) in value, identity in gradient."""
    return v + (v.detach().float().bfloat16().double() - v.detach())


def near_tie(v, got):
    """bf16(v), except where the kernel's value `got` is the other bf16 neighbour of v and v lies on the boundary between the two: got is
    no further from v than bf16(v) is, plus a slack of SLACK (1 + |v|) -- what fp32 arithmetic on operands of that size can move v by -- and
    never more than a quarter of v's bf16 ulp (|v| < 2^-7).  So only a value within 3/4 ulp of v is ever taken, one of the two bf16 values
    around v, and only where v is within ulp / 8 of their midpoint.  got = None: bf16(v)."""
    r = v.float().bfloat16().double()
    if got is None:
        return r
    gd = got.double()
    ulp = torch.ldexp(torch.ones_like(v), torch.frexp(v)[1] - 8)           # |v| in [2^(e-1), 2^e): 8 significant bits
    slack = torch.minimum(SLACK * (1 + v.abs()), ulp / 4)
    return torch.where((gd - v).abs() <= (r - v).abs() + slack, gd, r)


class RoundGrad(torch.autograd.Function):
    """Identity forward; the gradient, once all its contributions are summed, is rounded to bf16 (near_tie against `got`).  `keep`, a dict,
    receives the pure rounding bf16(gradient) under "dy_pure"."""
    @staticmethod
    def forward(ctx, v, got, keep):
        ctx.got, ctx.keep = got, keep
        return v.view_as(v)

    @staticmethod
    def backward(ctx, gr):
        ctx.keep["dy_pure"] = gr.float().bfloat16()
        return near_tie(gr, ctx.got), None, None


def ref_ln(xn, w, b, eps=EPS):
    mean = xn.mean(dim=-1, keepdim=True)
    var = (xn - mean).pow(2).mean(dim=-1, keepdim=True)
    rstd = torch.rsqrt(var + eps)
    return (xn - mean) * rstd * w + b, {"mean": mean[:, 0].detach(), "var": var[:, 0].detach(), "rstd": rstd[:, 0].detach()}


def ref_mix_chain(B, T, x, delta, w, b, mus, douts, d3b, first, y_prev, dy_last, y_got=None, dy_got=None):
    """add + LayerNorm + token shift + lerps and its backward.  Returns a dict of references.  y_got / dy_got: the kernels' bf16 LayerNorm output and
    its gradient, for near_tie."""
    ntok, C = x.shape
    xd, wd, bd = f64([x, w, b])
    md = f64(mus)
    xn = ste(xd + delta.double()) if delta is not None else xd
    yf, st = ref_ln(xn, wd, bd)
    yq = yf + (near_tie(yf.detach(), y_got) - yf.detach())
    yq.retain_grad()
    keep = {}
    y = RoundGrad.apply(yq, dy_got, keep)
    yp = (y_prev.double() if y_prev is not None else torch.zeros(B, C, dtype=torch.float64, device=x.device)).requires_grad_(True)
    n = torch.arange(ntok, device=x.device)
    opens = (n % T == 0)[:, None]
    sh = torch.cat([torch.zeros(1, C, dtype=torch.float64, device=x.device), y[:-1]])
    sh = torch.where(opens, yp.repeat_interleave(T, dim=0), sh)
    if first is not None:
        sh = torch.where((first != 0)[:, None] & ~opens, torch.zeros_like(sh), sh)
    outs = [y + (sh - y) * m for m in md]
    gr = [d.double() for d in douts]
    if d3b is not None:
        gr[3] = gr[3] + d3b.double()
    if dy_last is not None:
        outs, gr = outs + [y[T - 1::T]], gr + [dy_last.double()]
    torch.autograd.backward(outs, gr)
    return {"xn": xn, "y": yq, "y_pure": yf.detach().float().bfloat16(), "dy_pure": keep["dy_pure"], "outs": outs[:len(md)], "st": st, "dy": yq.grad, "dx": xd.grad, "dw": wd.grad, "db": bd.grad,
            "dmu": [m.grad for m in md], "dy_prev": yp.grad}


# ------------------------------------------------------------------------------------------------ add_ln
ADD_LN_FWD = [L, I, F32] + [VP] * 8
ADD_LN_BWD = [L, I] + [VP] * 9


def add_ln_fwd(be, ntok, C, x, delta, w, b):
    res = {"y": nan_rows(be, ntok, C), "mean": nan_rows(be, ntok, 1, torch.float32), "rstd": nan_rows(be, ntok, 1, torch.float32)}
    if delta is not None:
        res["xn"] = nan_rows(be, ntok, C)
    be.call("vrwkv_add_ln_fwd_bf16", ADD_LN_FWD, ntok, C, EPS, P(x), P(delta), P(w), P(b), P(res.get("xn")), P(res["y"]), P(res["mean"]), P(res["rstd"]))
    written(res, None, 0)
    return res


def host_fwd(x, delta, w, b):
    """What add_ln_fwd returns, computed here, a guard row included: the input of a backward kernel that is run alone.  The statistics are the
    fp64 ones rounded to fp32; y is what the backward kernels recompute from them, in their arithmetic: bf16(fma((xn - mean) rstd, w, b)) with
    fp32 operations (the product and the sum of the fma are exact in fp64)."""
    xn = x if delta is None else (x.float() + delta.float()).bfloat16()
    _, st = ref_ln(xn.double(), w.double(), b.double())
    mean, rstd = st["mean"].float()[:, None], st["rstd"].float()[:, None]
    y = (((xn.float() - mean) * rstd).double() * w.double() + b.double()).float().bfloat16()
    pad = lambda t: torch.cat([t, torch.full_like(t[:1], float("nan"))])
    return {"xn": pad(xn), "y": pad(y), "mean": pad(mean), "rstd": pad(rstd)}


def add_ln_bwd(be, ntok, C, dy, dres, xn, mean, rstd, w):
    res = {"dx": nan_rows(be, ntok, C), "dwb": nan_rows(be, 2, C, torch.float32)}
    used = be.ws("vrwkv_add_ln_ws_floats", ntok, C)
    assert used == min(ntok, LN_BWD_GRID) * 2 * C
    ws = nan_ws(be, used, C)
    be.call("vrwkv_add_ln_bwd_bf16", ADD_LN_BWD, ntok, C, P(dy), P(dres), P(xn), P(mean), P(rstd), P(w), P(res["dx"]), P(res["dwb"]), P(ws))
    written(res, ws, used)
    return res


@pytest.mark.parametrize("backend,sid,cfg", _cases(["plain", "delta", "dres", "delta+dres"], ["delta+dres"], emu_heavy=("deep",)))
def test_add_ln(backend, be, sid, cfg):
    B, T, C = be.shape(sid)
    ntok = B * T
    g = be.gen(17 * ntok + C + len(cfg))
    x, w, b, dy = rnd(be, g, ntok, C), rnd(be, g, C, scale=0.5, shift=1.0), rnd(be, g, C, scale=0.3), rnd(be, g, ntok, C)
    delta = rnd(be, g, ntok, C, scale=0.5) if "delta" in cfg else None
    dres = rnd(be, g, ntok, C) if "dres" in cfg else None
    edges(x, delta)
    tag = f"add_ln/{sid}/{cfg}"

    heavy = be.name == "emu" and sid in EMU_HEAVY           # the backward alone, once, on a forward computed here

    def run():
        f = host_fwd(x, delta, w, b) if heavy else add_ln_fwd(be, ntok, C, x, delta, w, b)
        r = add_ln_bwd(be, ntok, C, dy, dres, f["xn"] if delta is not None else x, f["mean"], f["rstd"], w)
        return {**f, **r}

    r1 = run()
    if not heavy:
        same_bits(r1, run())
    xd, wd, bd = f64([x, w, b])
    xn = ste(xd + delta.double()) if delta is not None else xd
    y, st = ref_ln(xn, wd, bd)
    y.backward(dy.double())
    if delta is not None:
        act(be, r1["xn"], xn, f"{tag} xn")
    act(be, r1["y"], y, f"{tag} y")
    stats(be, r1["mean"], r1["rstd"], st, tag)
    act(be, r1["dx"], xd.grad + (dres.double() if dres is not None else 0), f"{tag} dx")
    par(be, r1["dwb"][0], wd.grad, f"{tag} dw")
    par(be, r1["dwb"][1], bd.grad, f"{tag} db")
    if ntok >= 3:        # the zero-variance row: y = b exactly where the row mean is exact, rstd = 1 / sqrt(eps)
        assert abs(float(r1["rstd"][ntok - 1, 0]) * EPS ** 0.5 - 1) < 1e-5 and abs(float(r1["rstd"][ntok // 2, 0]) * EPS ** 0.5 - 1) < 1e-5
        assert torch.equal(bits(r1["y"][ntok // 2]), bits(b)), f"{tag}: the all-zero row is not b"


@pytest.mark.parametrize("backend,sid,cfg", _cases(["plain", "delta", "delta+dscale"], ["delta+dscale"]))
def test_add_ln_scaled_fwd(backend, be, sid, cfg):
    B, T, C = be.shape(sid)
    ntok = B * T
    g = be.gen(19 * ntok + C + len(cfg))
    x, w, b = rnd(be, g, ntok, C), rnd(be, g, C, scale=0.5, shift=1.0), rnd(be, g, C, scale=0.3)
    delta = rnd(be, g, ntok, C, scale=0.5) if "delta" in cfg else None
    dscale = rnd(be, g, C, scale=0.5) if "dscale" in cfg else None
    edges(x, delta)
    tag = f"add_ln_scaled/{sid}/{cfg}"

    def run():
        res = {"y": nan_rows(be, ntok, C)}
        if delta is not None:
            res["xn"] = nan_rows(be, ntok, C)
        be.call("vrwkv_add_ln_scaled_fwd_bf16", [L, I, F32] + [VP] * 7, ntok, C, EPS, P(x), P(delta), P(dscale), P(w), P(b), P(res.get("xn")), P(res["y"]))
        written(res, None, 0)
        return res

    r1, r2 = run(), run()
    same_bits(r1, r2)
    xn = x.double()
    if delta is not None:       # one fma before the rounding: the product and the sum are exact in fp64
        xn = ste(xn + delta.double() * (dscale.double() if dscale is not None else 1.0))
        act(be, r1["xn"], xn, f"{tag} xn")
    y, _ = ref_ln(xn, w.double(), b.double())
    act(be, r1["y"], y, f"{tag} y")
    if cfg != "delta+dscale":   # without a scale the entry is add_ln_fwd without its statistics
        same_bits({k: r1[k] for k in r1}, {k: v for k, v in add_ln_fwd(be, ntok, C, x, delta, w, b).items() if k in r1})


# ------------------------------------------------------------------------------------------------ scatter / gather
@pytest.mark.parametrize("backend,sid", [pytest.param(*c.values, id=c.id, marks=c.marks) for c in _cases()
                                         if c.values[1] in ("one_token", "caps", "partial_wave", "lb512_first", "lb1024_full", "x_wide_1024")])
def test_ln_scatter_gather(backend, be, sid):
    """out[row_index[n]] = LN(x[n]) into a larger NaN-prefilled tensor and its backward; negative entries drop their row."""
    B, T, C = be.shape(sid)
    ntok = B * T                                            # `caps`: 1125 rows, G = 1024
    nout = ntok + 7
    g = be.gen(23 * ntok + C)
    x, w, b, dout = rnd(be, g, ntok, C), rnd(be, g, C, scale=0.5, shift=1.0), rnd(be, g, C, scale=0.3), rnd(be, g, nout, C)
    edges(x, None)
    idx = torch.randperm(nout, generator=torch.Generator().manual_seed(ntok))[:ntok].to(torch.int64)
    dropped = sorted({0, ntok // 3, ntok - 1}) if ntok >= 3 else []
    for k, n in enumerate(dropped):
        idx[n] = -1 - k
    idx = idx.to(be.dev)
    keep = idx >= 0
    tag = f"scatter/{sid}"

    def run():
        res = {"out": nan_rows(be, nout, C), "mean": nan_rows(be, ntok, 1, torch.float32), "rstd": nan_rows(be, ntok, 1, torch.float32),
               "dx": nan_rows(be, ntok, C), "dwb": nan_rows(be, 2, C, torch.float32)}
        be.call("vrwkv_ln_scatter_fwd_bf16", [L, I, F32] + [VP] * 7, ntok, C, EPS, P(x), P(w), P(b), P(idx), P(res["out"]), P(res["mean"]), P(res["rstd"]))
        used = be.ws("vrwkv_add_ln_ws_floats", ntok, C)
        ws = nan_ws(be, used, C)
        be.call("vrwkv_ln_gather_bwd_bf16", [L, I] + [VP] * 9, ntok, C, P(dout), P(idx), P(x), P(res["mean"]), P(res["rstd"]), P(w), P(res["dx"]), P(res["dwb"]), P(ws))
        written({k: v for k, v in res.items() if k != "out"}, ws, used)
        return res

    r1, r2 = run(), run()
    same_bits(r1, r2)
    named = torch.zeros(nout + 1, dtype=torch.bool, device=be.dev)
    named[idx[keep]] = True
    nan = torch.full((C,), float("nan"), dtype=torch.bfloat16, device=be.dev)
    assert bool((bits(r1["out"][~named]) == bits(nan)).all()), f"{tag}: a row that no index names was written"
    xd, wd, bd = f64([x, w, b])
    y, st = ref_ln(xd, wd, bd)
    y[keep].backward(dout[idx[keep]].double())
    act(be, r1["out"][idx[keep]], y[keep], f"{tag} out", guard=False)
    stats(be, r1["mean"], r1["rstd"], st, tag)
    act(be, r1["dx"], xd.grad, f"{tag} dx")
    assert not bool(r1["dx"][:-1][~keep].any()), f"{tag}: a dropped row has a gradient"
    par(be, r1["dwb"][0], wd.grad, f"{tag} dw")
    par(be, r1["dwb"][1], bd.grad, f"{tag} db")


# ------------------------------------------------------------------------------------------------ ln_mix / mix_bwd_ln
def _ln_mix_fwd(be, form, ntok, T, C, M, x, delta, w, b, mus, first, y_prev, want_y_last):
    B = ntok // T
    outs = [nan_rows(be, ntok, C) for _ in range(M)]
    res = {"mean": nan_rows(be, ntok, 1, torch.float32), "rstd": nan_rows(be, ntok, 1, torch.float32), **{f"out{j}": o for j, o in enumerate(outs)}}
    if delta is not None:
        res["xn"] = nan_rows(be, ntok, C)
    if want_y_last:
        res["y_last"] = nan_rows(be, B, C)
    head = [ntok, T, C, EPS, M, P(x), P(delta), P(w), P(b), PA(mus), P(res.get("xn")), PA(outs), P(res["mean"]), P(res["rstd"])]
    types = [L, I, I, F32, I] + [VP] * 9
    if form == "plain":
        be.call("vrwkv_ln_mix_fwd_bf16", types, *head)
    elif form == "packed":
        be.call("vrwkv_ln_mix_fwd_packed_bf16", types + [VP], *head, P(first))
    else:
        be.call("vrwkv_ln_mix_fwd_carry_bf16", types + [VP, VP], *head, P(y_prev), P(res.get("y_last")))
    written(res, None, 0)
    return res


def _token_shift_bwd(be, form, ntok, T, C, M, xn, f, w, b, mus, douts, d3b, dres, first, y_prev, dy_last, want_dy_prev, chain=True):
    """M = 1: ln_mix_bwd.  M = 6: mix_bwd_ln, then (chain) add_ln_bwd on its dx -- the product's time-mix backward."""
    B = ntok // T
    res = {"dmu": nan_rows(be, M, C, torch.float32)}
    if want_dy_prev:
        res["dy_prev"] = nan_rows(be, B, C, torch.float32)
    tail = {"plain": [], "packed": [P(first)], "carry": [P(y_prev), P(dy_last), P(res.get("dy_prev"))]}[form]
    sfx = {"plain": "", "packed": "_packed", "carry": "_carry"}[form]
    if M == 1:
        res.update(dx=nan_rows(be, ntok, C), dwb=nan_rows(be, 2, C, torch.float32))
        used = be.ws("vrwkv_ln_mix_ws_floats", ntok, C, M)
        assert used == min(ntok, LN_MIX_BWD_GRID) * (2 + M) * C
        ws = nan_ws(be, used, C)
        be.call(f"vrwkv_ln_mix_bwd{sfx}_bf16", [L, I, I, I] + [VP] * (13 + len(tail)), ntok, T, C, M, P(xn), P(f["mean"]), P(f["rstd"]), P(w), P(b),
                PA(mus), PA(douts), None, P(dres), *tail, P(res["dx"]), P(res["dwb"]), P(res["dmu"]), P(ws))
        written(res, ws, used)
        return res
    res["dy"] = nan_rows(be, ntok, C)
    used = be.ws("vrwkv_param_grad_ws_floats", ntok, C, M)
    assert used == min((ntok + MIX_TPB - 1) // MIX_TPB, MIX_BWD_GRID) * M * C
    ws = nan_ws(be, used, C)
    be.call(f"vrwkv_mix_bwd_ln{sfx}_bf16", [L, I, I, I] + [VP] * (11 + len(tail)), ntok, T, C, M, P(xn), P(f["mean"]), P(f["rstd"]), P(w), P(b),
            PA(mus), PA(douts), P(d3b), *tail, P(res["dy"]), P(res["dmu"]), P(ws))
    written(res, ws, used)
    if chain:
        res.update(add_ln_bwd(be, ntok, C, res["dy"], dres, xn, f["mean"], f["rstd"], w))
    return res


def _mix_case(be, sid, M, cfg):
    """cfg: plain | packed | packed:null | carry:<subset of p = y_prev, l = y_last (forward) and dy_last (backward), d = dy_prev>, then
    +dres (a residual gradient), +dup3 (M = 6: dout3_second), +nodelta (xn = x)."""
    B, T, C = be.shape(sid)
    ntok = B * T
    base, *opts = cfg.split("+")
    form, _, sub = base.partition(":")
    bwd_only = be.name == "emu" and sid in EMU_HEAVY          # ln_mix_bwd (once) / mix_bwd_ln alone, on host_fwd
    g = be.gen(1000 * M + 7 * ntok + C + sum(map(ord, cfg)))
    x, w, b = rnd(be, g, ntok, C), rnd(be, g, C, scale=0.5, shift=1.0), rnd(be, g, C, scale=0.3)
    delta = None if "nodelta" in opts else rnd(be, g, ntok, C, scale=0.5)
    edges(x, delta)
    mus = [unif(be, g, C) for _ in range(M)]
    douts = [rnd(be, g, ntok, C) for _ in range(M)]
    d3b = rnd(be, g, ntok, C) if "dup3" in opts else None
    dres = rnd(be, g, ntok, C) if "dres" in opts else None
    first = draw_first(be, ntok, T, M) if form == "packed" and sub != "null" else None
    y_prev = rnd(be, g, B, C) if "p" in sub and form == "carry" else None
    dy_last = torch.randn(B, C, generator=g, device=be.dev) if "l" in sub and form == "carry" else None
    want_l, want_d = form == "carry" and "l" in sub, form == "carry" and "d" in sub
    tag = f"{'ln_mix' if M == 1 else 'mix_bwd_ln'}/{sid}/{cfg}"

    # where the sample and segment starts fall in each kernel's ranges
    starts = set(range(0, ntok, T)) | (set(torch.nonzero(first.cpu())[:, 0].tolist()) if first is not None else set())
    for kern, G in grids(ntok, M).items():
        kinds = start_kinds(ntok, G, starts)
        if first is None and (sid, kern) in PLAIN_STARTS:
            assert PLAIN_STARTS[(sid, kern)] <= kinds, (tag, kern, G, kinds)
        if first is not None and sid in PACKED_STARTS:
            assert {"lo", "inside", "hi"} <= kinds, (tag, kern, G, kinds)
    if first is not None and ntok >= 4:
        assert bool(first[ntok // 2]) and bool(first[ntok // 2 + 1])          # the one-token segment

    # the two-kernel path's forward: the LayerNorm output that the fused kernels never store
    yk = host_fwd(x, delta, w, b) if bwd_only else add_ln_fwd(be, ntok, C, x, delta, w, b)

    def run(fm):
        if bwd_only:
            return _token_shift_bwd(be, fm, ntok, T, C, M, yk["xn"] if delta is not None else x, yk, w, b, mus, douts, d3b, dres, first, y_prev, dy_last,
                                    want_d, chain=False)
        f = _ln_mix_fwd(be, fm, ntok, T, C, M, x, delta, w, b, mus, first, y_prev, want_l)
        r = _token_shift_bwd(be, fm, ntok, T, C, M, f["xn"] if delta is not None else x, f, w, b, mus, douts, d3b, dres, first, y_prev, dy_last, want_d)
        return {**f, **r}

    r1 = run(form)
    if not (bwd_only and M == 1):
        same_bits(r1, run(form))
    if base in ("packed:null", "carry:"):                 # no marks / no carry pointers: the plain entry, bit for bit
        same_bits(r1, run("plain"))

    ref = ref_mix_chain(B, T, x, delta, w, b, mus, douts, d3b, first, y_prev, dy_last, yk["y"][:-1], r1["dy"][:-1] if M == 6 else None)
    act(be, yk["y"], ref["y_pure"], f"{tag} y")
    for j in range(M):
        if not bwd_only:
            act(be, r1[f"out{j}"], ref["outs"][j], f"{tag} out{j}")
        par(be, r1["dmu"][j], ref["dmu"][j], f"{tag} dmu{j}")
    if M == 6:
        act(be, r1["dy"], ref["dy_pure"], f"{tag} dy")
    if want_d:
        for s in range(B):
            par(be, r1["dy_prev"][s], ref["dy_prev"][s], f"{tag} dy_prev[{s}]")
    if bwd_only:
        if M == 1:
            act(be, r1["dx"], ref["dx"] + (dres.double() if dres is not None else 0), f"{tag} dx")
            par(be, r1["dwb"][0], ref["dw"], f"{tag} dw")
            par(be, r1["dwb"][1], ref["db"], f"{tag} db")
        return
    for k in ("mean", "rstd") + (("xn",) if delta is not None else ()):       # the fused forward saves what the two-kernel path saves
        assert torch.equal(bits(r1[k]), bits(yk[k])), f"{tag} {k}: differs from add_ln_fwd"
    if delta is not None:
        act(be, r1["xn"], ref["xn"], f"{tag} xn")
    stats(be, r1["mean"], r1["rstd"], ref["st"], tag)
    if want_l:
        act(be, r1["y_last"], ref["y"][T - 1::T], f"{tag} y_last")
    act(be, r1["dx"], ref["dx"] + (dres.double() if dres is not None else 0), f"{tag} dx")
    par(be, r1["dwb"][0], ref["dw"], f"{tag} dw")
    par(be, r1["dwb"][1], ref["db"], f"{tag} db")
    if sid in FULL_MATRIX and cfg not in ("plain", "packed", "carry:p", "carry:pl"):
        return

    # exact shift indexing: with mu = 1 every output is the LayerNorm output of the row before, zeros at a start, the carried row at a carried start
    wq, bq = torch.full_like(w, 0.25), torch.full_like(b, 3.0)
    ones = [torch.ones(C, dtype=torch.bfloat16, device=be.dev) for _ in range(M)]
    y = add_ln_fwd(be, ntok, C, x, delta, wq, bq)["y"][:-1]
    sh = torch.cat([torch.zeros_like(y[:1]), y[:-1]])
    opens = torch.zeros(ntok, dtype=torch.bool, device=be.dev)
    opens[::T] = True
    yp = (y_prev.float() * 0.25 + 3.0).bfloat16() if y_prev is not None else None          # in the range of y, like a real carried row
    sh[opens] = yp if yp is not None else torch.zeros(B, C, dtype=torch.bfloat16, device=be.dev)
    if first is not None:
        sh[first != 0] = 0
    o = _ln_mix_fwd(be, form, ntok, T, C, M, x, delta, wq, bq, ones, first, yp, want_l)
    for j in range(M):
        assert torch.equal(bits(o[f"out{j}"][:-1]), bits(sh)), f"{tag} out{j}: shifted rows"
    if want_l:
        assert torch.equal(bits(o["y_last"][:-1]), bits(y[T - 1::T])), f"{tag}: y_last"


CARRY = ["carry:" + "".join(s for s, on in zip("pld", (a, b, c)) if on) for a in (0, 1) for b in (0, 1) for c in (0, 1)]
M1_ALL = ["plain", "plain+dres", "plain+dres+nodelta", "packed", "packed+dres", "packed:null"] + CARRY[:-1] + ["carry:pld+dres"]
M6_ALL = ["plain", "plain+dup3", "plain+dres+nodelta", "packed", "packed+dup3+dres", "packed:null"] + CARRY[:-1] + ["carry:pld+dup3"]


@pytest.mark.parametrize("backend,sid,cfg", _cases(M1_ALL, ["plain+dres", "packed", "carry:pld"], shift=True, emu_heavy=("deep",)))
def test_ln_mix(backend, be, sid, cfg):
    """ln_mix_fwd (M = 1) and ln_mix_bwd, plain / packed / carry."""
    _mix_case(be, sid, 1, cfg)


@pytest.mark.parametrize("backend,sid,cfg", _cases(M6_ALL, ["plain+dup3", "packed+dres", "carry:pld"], shift=True, emu_heavy=EMU_HEAVY))
def test_mix_bwd_ln(backend, be, sid, cfg):
    """ln_mix_fwd (M = 6), mix_bwd_ln and add_ln_bwd on its dx, plain / packed / carry."""
    _mix_case(be, sid, 6, cfg)


# ------------------------------------------------------------------------------------------------ argument checks
@pytest.mark.parametrize("backend", BACKENDS)
def test_arguments(backend, be):
    """What the entries refuse, by return code; nothing is launched."""
    ntok, T, C = 8, 4, 64
    t = torch.zeros(64, 64, dtype=torch.float32, device=be.dev)
    p, arr = P(t), PA([t] * 6)
    lib = {
        "add_ln_fwd": ("vrwkv_add_ln_fwd_bf16", ADD_LN_FWD, [ntok, C, EPS, p, p, p, p, p, p, p, p], (3, 5, 6, 8, 9, 10)),
        "add_ln_scaled_fwd": ("vrwkv_add_ln_scaled_fwd_bf16", [L, I, F32] + [VP] * 7, [ntok, C, EPS, p, p, p, p, p, p, p], (3, 6, 7, 9)),
        "ln_scatter_fwd": ("vrwkv_ln_scatter_fwd_bf16", [L, I, F32] + [VP] * 7, [ntok, C, EPS, p, p, p, p, p, p, p], (3, 4, 5, 6, 7, 8, 9)),
        "ln_gather_bwd": ("vrwkv_ln_gather_bwd_bf16", [L, I] + [VP] * 9, [ntok, C, p, p, p, p, p, p, p, p, p], tuple(range(2, 11))),
        "add_ln_bwd": ("vrwkv_add_ln_bwd_bf16", ADD_LN_BWD, [ntok, C, p, p, p, p, p, p, p, p, p], (2, 4, 5, 6, 7, 8, 9, 10)),
        "ln_mix_fwd": ("vrwkv_ln_mix_fwd_bf16", [L, I, I, F32, I] + [VP] * 9, [ntok, T, C, EPS, 1, p, p, p, p, arr, p, arr, p, p], (5, 7, 8, 9, 11, 12, 13)),
        "ln_mix_fwd_packed": ("vrwkv_ln_mix_fwd_packed_bf16", [L, I, I, F32, I] + [VP] * 10, [ntok, T, C, EPS, 1, p, p, p, p, arr, p, arr, p, p, p], (5, 7, 8, 9, 11, 12, 13)),
        "ln_mix_fwd_carry": ("vrwkv_ln_mix_fwd_carry_bf16", [L, I, I, F32, I] + [VP] * 11, [ntok, T, C, EPS, 1, p, p, p, p, arr, p, arr, p, p, p, p], (5, 7, 8, 9, 11, 12, 13)),
        "ln_mix_bwd": ("vrwkv_ln_mix_bwd_bf16", [L, I, I, I] + [VP] * 13, [ntok, T, C, 1, p, p, p, p, p, arr, arr, None, p, p, p, p, p], (4, 5, 6, 7, 8, 9, 10, 13, 14, 15, 16)),
        "ln_mix_bwd_packed": ("vrwkv_ln_mix_bwd_packed_bf16", [L, I, I, I] + [VP] * 14, [ntok, T, C, 1, p, p, p, p, p, arr, arr, None, p, p, p, p, p, p], (4, 5, 6, 7, 8, 9, 10, 14, 15, 16, 17)),
        "ln_mix_bwd_carry": ("vrwkv_ln_mix_bwd_carry_bf16", [L, I, I, I] + [VP] * 16, [ntok, T, C, 1, p, p, p, p, p, arr, arr, None, p, p, p, p, p, p, p, p], (4, 5, 6, 7, 8, 9, 10, 16, 17, 18, 19)),
        "mix_bwd_ln": ("vrwkv_mix_bwd_ln_bf16", [L, I, I, I] + [VP] * 11, [ntok, T, C, 6, p, p, p, p, p, arr, arr, p, p, p, p], (4, 5, 6, 7, 8, 9, 10, 12, 13, 14)),
        "mix_bwd_ln_packed": ("vrwkv_mix_bwd_ln_packed_bf16", [L, I, I, I] + [VP] * 12, [ntok, T, C, 6, p, p, p, p, p, arr, arr, p, p, p, p, p], (4, 5, 6, 7, 8, 9, 10, 13, 14, 15)),
        "mix_bwd_ln_carry": ("vrwkv_mix_bwd_ln_carry_bf16", [L, I, I, I] + [VP] * 14, [ntok, T, C, 6, p, p, p, p, p, arr, arr, p, p, p, p, p, p, p], (4, 5, 6, 7, 8, 9, 10, 15, 16, 17)),
    }

    def rc(name, **change):
        fn, types, args, _ = lib[name]
        args = list(args)
        for k, v in change.items():
            args[int(k[1:])] = v
        return be.rc(fn, types, *args)

    for name, (fn, types, args, required) in lib.items():
        ci = 2 if "mix" in name else 1
        for c in (96, 8256):
            assert rc(name, **{f"a{ci}": c}) == ESHAPE, (name, "C", c)
        assert rc(name, a0=0) == EINVAL, (name, "ntok = 0")
        for k in required:                                   # a NULL among the required pointers
            assert rc(name, **{f"a{k}": None}) == EINVAL, (name, "NULL argument", k)
        if "mix" in name:
            assert rc(name, a0=ntok + 1) in (EINVAL, ESHAPE), (name, "ntok % T")
            mi = 4 if "fwd" in name else 3
            for j in range(args[mi]):                        # a NULL inside mu[] / out[] / dout[]
                holed = (VP * 6)(*[t.data_ptr() if i != j else None for i in range(6)])
                for k in ((9, 11) if "fwd" in name else (9, 10)):
                    assert rc(name, **{f"a{k}": holed}) == EINVAL, (name, "NULL in array", k, j)
    for name in ("ln_mix_fwd", "ln_mix_fwd_packed", "ln_mix_fwd_carry"):
        for m in (0, 2, 5, 7):
            assert rc(name, a4=m) == ESHAPE, (name, "M", m)
        assert rc(name, a10=None) == EINVAL, (name, "delta without xn")
        assert rc(name, a0=ntok + 1) == EINVAL
    for name in ("ln_mix_bwd", "ln_mix_bwd_packed", "ln_mix_bwd_carry"):
        for m in (0, 2, 6, 7):
            assert rc(name, a3=m) == ESHAPE, (name, "M", m)
        assert rc(name, a11=p) == ESHAPE, (name, "dout3_second")
        assert rc(name, a0=ntok + 1) == EINVAL
    for name in ("mix_bwd_ln", "mix_bwd_ln_packed", "mix_bwd_ln_carry"):
        for m in (0, 1, 2, 7):
            assert rc(name, a3=m) == EINVAL, (name, "M", m)
        assert rc(name, a0=ntok + 1) == ESHAPE
    assert rc("add_ln_fwd", a7=None) == EINVAL                # delta without xn
    assert rc("add_ln_scaled_fwd", a8=None) == EINVAL
    assert rc("add_ln_scaled_fwd", a4=None, a8=None) == EINVAL        # dscale without delta
