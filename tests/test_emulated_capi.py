"""The WKV7 C entry points themselves (csrc/wkv7_capi.hip compiled whole for the host emulator): what the GPU parity tests call
through the product library, called here on CPU tensors -- the launchers' kernel selection (few heads: two workgroups per head in the
forward; the backward's default and variant 5; batch slices above the 32-bit offset limit), the argument checks, and the kernels behind them against the C oracle."""
import ctypes

import pytest
import torch

from oracle import wkv7_c
from oracle.wkv7_oracle import make_inputs, rel_rms
from tests.state_ref import DS_TOL, check_grads, reference, rel_rms64, state_inputs

I, VP = ctypes.c_int, ctypes.c_void_p
TOL = 1e-3          # north_star: 1e-3 against the oracle rounded to bf16 the same way
EINVAL, ESHAPE, EALIGN = -1, -2, -3      # include/visualrwkv_hip.h


def P(t):
    return VP(t.data_ptr()) if t is not None else VP(0)


def _fwd(lib, w, q, k, v, z, a):
    B, T, H, N = w.shape
    y = torch.zeros_like(v)
    s = torch.zeros(B, H, T // 16, N, N)
    sa = torch.zeros(B, T, H, N)
    lib.vrwkv_wkv7_forward_bf16.argtypes = [I, I, I] + [VP] * 10
    rc = lib.vrwkv_wkv7_forward_bf16(B, T, H, *[P(x) for x in (w, q, k, v, z, a, y, s, sa)], None)
    assert rc == 0, rc
    return y, s, sa


def _bwd(lib, w, q, k, v, z, a, dy, s, sa):
    B, T, H, N = w.shape
    outs = [torch.zeros_like(w) for _ in range(6)]
    lib.vrwkv_wkv7_backward_bf16.argtypes = [I, I, I] + [VP] * 16
    rc = lib.vrwkv_wkv7_backward_bf16(B, T, H, *[P(x) for x in (w, q, k, v, z, a, dy, s, sa)], *[P(o) for o in outs], None)
    assert rc == 0, rc
    return outs


@pytest.mark.parametrize("B,T,H", [(1, 16, 1), (2, 48, 2)])
def test_forward_and_backward_through_the_c_entries(emu_lib, B, T, H):
    w, q, k, v, z, a, dy = make_inputs(B, T, H, seed=B * 7 + T)
    yr, sr, sar = wkv7_c.forward(w, q, k, v, z, a)
    y, s, sa = _fwd(emu_lib, w, q, k, v, z, a)                     # B * H <= 128: the launcher picks two workgroups per head
    assert rel_rms(y.float(), yr.float()) < TOL
    assert rel_rms(s, sr) < 2e-5 and rel_rms(sa, sar) < 2e-5
    ref = wkv7_c.backward(w, q, k, v, z, a, dy, sr, sar)
    for variant in (-1, 5):                                          # default = 8 at these sizes (wkv7_bwd_v8.h), 5 = wkv7_bwd_v5.h
        assert emu_lib.vrwkv_wkv7_set_backward_variant(variant) == 0
        try:
            outs = _bwd(emu_lib, w, q, k, v, z, a, dy, sr, sar)
        finally:
            emu_lib.vrwkv_wkv7_set_backward_variant(-1)
        for n, o, r in zip(("dw", "dq", "dk", "dv", "dz", "da"), outs, ref):
            assert rel_rms(o.float(), r.float()) < TOL, (variant, n)


def test_backward_batch_slices_on_the_host(emu_lib):
    """The launcher's batch slicing (tensors of 4 GiB and more in production; the limit lowered here): 3 samples as slices of 2 + 1 are
    bit-identical to one launch, a single sample above the limit goes to the 64-bit kernel (variant 5)."""
    B, T, H = 3, 32, 2
    w, q, k, v, z, a, dy = make_inputs(B, T, H, seed=91)
    _, sr, sar = wkv7_c.forward(w, q, k, v, z, a)
    ref = wkv7_c.backward(w, q, k, v, z, a, dy, sr, sar)
    per_sample = T * H * 64 * 4
    emu_lib.vrwkv_wkv7_set_backward_slice_limit.argtypes = [ctypes.c_ulonglong]
    try:
        base = _bwd(emu_lib, w, q, k, v, z, a, dy, sr, sar)
        assert emu_lib.vrwkv_wkv7_set_backward_slice_limit(2 * per_sample + 1) == 0
        sliced = _bwd(emu_lib, w, q, k, v, z, a, dy, sr, sar)
        assert emu_lib.vrwkv_wkv7_last_variant(1) == 8
        for o, r in zip(sliced, base):
            assert torch.equal(o, r)
        assert emu_lib.vrwkv_wkv7_set_backward_slice_limit(per_sample // 2) == 0
        wide = _bwd(emu_lib, w, q, k, v, z, a, dy, sr, sar)
        assert emu_lib.vrwkv_wkv7_last_variant(1) == 5
        for o, r in zip(wide, ref):
            assert rel_rms(o.float(), r.float()) < TOL
    finally:
        emu_lib.vrwkv_wkv7_set_backward_slice_limit(0)


def test_argument_checks_of_the_launchers(emu_lib):
    w, q, k, v, z, a, dy = make_inputs(1, 16, 1, seed=3)
    y, s, sa = torch.zeros_like(v), torch.zeros(1, 1, 1, 64, 64), torch.zeros(1, 16, 1, 64)
    f = emu_lib.vrwkv_wkv7_forward_bf16
    f.argtypes = [I, I, I] + [VP] * 10
    assert f(1, 15, 1, *[P(x) for x in (w, q, k, v, z, a, y, s, sa)], None) != 0            # T % 16
    assert f(1, 16, 1, P(w), None, *[P(x) for x in (k, v, z, a, y, s, sa)], None) != 0      # null pointer
    assert emu_lib.vrwkv_wkv7_set_backward_variant(4) != 0                                   # dropped generations
    for v in (6, 7, 10, 11, 61, 81):                                                            # A/B partners live in benchmarks/experiments, not in the product launcher
        assert emu_lib.vrwkv_wkv7_set_backward_variant(v) != 0
    assert emu_lib.vrwkv_wkv7_last_variant(0) in (0, 4, 6, 7) and emu_lib.vrwkv_wkv7_last_variant(1) in (0, 5, 8, 9)
    assert emu_lib.vrwkv_wkv7_set_backward_variant(-1) == 0


def _entry(lib, name, n_int, n_ptr):
    fn = getattr(lib, name)
    fn.argtypes = [I] * n_int + [VP] * (n_ptr + 1)          # + the stream
    return fn


def _fwd_state(lib, ins, s0):
    B, T, H, N = ins[0].shape
    y, fin = torch.zeros_like(ins[3]), torch.zeros(B, H, N, N)
    s, sa = torch.zeros(B, H, T // 16, N, N), torch.zeros(B, T, H, N)
    rc = _entry(lib, "vrwkv_wkv7_forward_state_bf16", 3, 11)(B, T, H, *[P(x) for x in (*ins, y, s0, fin, s, sa)], None)
    assert rc == 0, rc
    return y, fin, s, sa


def _bwd_state(lib, ins, dy, s, sa, s0, ds_final):
    B, T, H, N = ins[0].shape
    outs, ds0 = [torch.zeros_like(ins[0]) for _ in range(6)], torch.zeros(B, H, N, N)
    rc = _entry(lib, "vrwkv_wkv7_backward_state_bf16", 3, 18)(B, T, H, *[P(x) for x in (*ins, dy, s, sa, s0, ds_final, ds0, *outs)], None)
    assert rc == 0, rc
    return outs, ds0


@pytest.mark.parametrize("variant", [-1, 9])                # -1: schedule 8 at this size
def test_state_backward_batch_slices_on_the_host(emu_lib, variant):
    """vrwkv_wkv7_backward_state_bf16 slices s0 / ds_final / ds0 per sample with the batch: 3 samples as slices of 2 + 1 are bit-identical to
    one launch; a single sample above the limit goes to the 64-bit kernel (variant 5), held to the limits of tests/state_ref.py."""
    B, T, H = 3, 32, 2
    ins, dy, s0, dsT = state_inputs(B, T, H, seed=92 + variant)
    _, _, s, sa = _fwd_state(emu_lib, ins, s0)
    _, _, gr, ds0r = reference(ins, dy, s0, dsT)
    per_sample = T * H * 64 * 4
    emu_lib.vrwkv_wkv7_set_backward_slice_limit.argtypes = [ctypes.c_ulonglong]
    assert emu_lib.vrwkv_wkv7_set_backward_variant(variant) == 0
    try:
        base, base_ds0 = _bwd_state(emu_lib, ins, dy, s, sa, s0, dsT)
        assert emu_lib.vrwkv_wkv7_set_backward_slice_limit(2 * per_sample + 1) == 0
        sliced, sliced_ds0 = _bwd_state(emu_lib, ins, dy, s, sa, s0, dsT)
        assert emu_lib.vrwkv_wkv7_last_variant(1) == (8 if variant == -1 else variant)
        for o, r in zip(sliced + [sliced_ds0], base + [base_ds0]):
            assert torch.equal(o, r)
        assert float(base_ds0[2].abs().max()) > 0               # the last slice wrote its own sample's state gradient
        assert emu_lib.vrwkv_wkv7_set_backward_slice_limit(per_sample // 2) == 0
        wide, wide_ds0 = _bwd_state(emu_lib, ins, dy, s, sa, s0, dsT)
        assert emu_lib.vrwkv_wkv7_last_variant(1) == 5
        check_grads(wide, gr, f"state, one sample above the limit, override {variant}", tol=TOL)
        assert rel_rms64(wide_ds0, ds0r) < DS_TOL
    finally:
        emu_lib.vrwkv_wkv7_set_backward_slice_limit(0)
        emu_lib.vrwkv_wkv7_set_backward_variant(-1)


PACKED_RESETS = [[1, 0], [1, 1], [0, 1]]                    # resets at chunks {0}, {0, 1}, {1}: another pattern in each of the three rows


def _bwd_packed(lib, ins, dy, s, sa, reset):
    B, T, H, _ = ins[0].shape
    outs = [torch.zeros_like(ins[0]) for _ in range(6)]
    rc = _entry(lib, "vrwkv_wkv7_backward_packed_bf16", 3, 16)(B, T, H, *[P(x) for x in (*ins, dy, s, sa, reset, *outs)], None)
    return rc, outs


@pytest.mark.parametrize("variant", [8, 9])
def test_packed_backward_batch_slices_on_the_host(emu_lib, variant):
    """vrwkv_wkv7_backward_packed_bf16 slices chunk_reset per row with the batch: slices of 2 + 1 are bit-identical to one launch.  A single
    sample above the limit has no packed kernel: VRWKV_ESHAPE, and nothing is recorded."""
    B, T, H = 3, 32, 2
    *ins, dy = make_inputs(B, T, H, seed=93 + variant)
    reset = torch.tensor(PACKED_RESETS, dtype=torch.uint8)
    y, s, sa = torch.zeros_like(ins[3]), torch.zeros(B, H, T // 16, 64, 64), torch.zeros(B, T, H, 64)
    assert _entry(emu_lib, "vrwkv_wkv7_forward_packed_bf16", 3, 10)(B, T, H, *[P(x) for x in (*ins, y, reset, s, sa)], None) == 0
    per_sample = T * H * 64 * 4
    emu_lib.vrwkv_wkv7_set_backward_slice_limit.argtypes = [ctypes.c_ulonglong]
    assert emu_lib.vrwkv_wkv7_set_backward_variant(variant) == 0
    try:
        rc, base = _bwd_packed(emu_lib, ins, dy, s, sa, reset)
        assert rc == 0 and emu_lib.vrwkv_wkv7_last_variant(1) == variant
        assert emu_lib.vrwkv_wkv7_set_backward_slice_limit(2 * per_sample + 1) == 0
        rc, sliced = _bwd_packed(emu_lib, ins, dy, s, sa, reset)
        assert rc == 0 and emu_lib.vrwkv_wkv7_last_variant(1) == variant
        for o, r in zip(sliced, base):
            assert torch.equal(o, r)
        assert emu_lib.vrwkv_wkv7_set_backward_variant(17 - variant) == 0        # the other schedule: a recording would show
        assert emu_lib.vrwkv_wkv7_set_backward_slice_limit(per_sample // 2) == 0
        rc, _ = _bwd_packed(emu_lib, ins, dy, s, sa, reset)
        assert rc == ESHAPE and emu_lib.vrwkv_wkv7_last_variant(1) == variant
    finally:
        emu_lib.vrwkv_wkv7_set_backward_slice_limit(0)
        emu_lib.vrwkv_wkv7_set_backward_variant(-1)


# The seven bf16 launch entries: name, extra ints after (B, T, H), and the pointer arguments in order -- "r": required, "o": optional
# (NULL allowed, alignment checked when given), "b": the byte array chunk_reset (NULL allowed, no alignment asked of it).
_ACTS_FWD, _ACTS_BWD, _GRADS = "w q k v z a y", "w q k v z a dy s sa", "dw dq dk dv dz da"
ENTRIES = {
    "vrwkv_wkv7_forward_bf16": ((), {"r": _ACTS_FWD + " s sa"}),
    "vrwkv_wkv7_forward_state_bf16": ((), {"r": _ACTS_FWD, "o": "s0 s_final s_ckpt sa"}),
    "vrwkv_wkv7_forward_packed_bf16": ((), {"r": _ACTS_FWD, "b": "chunk_reset", "o": "s_ckpt sa"}),
    "vrwkv_wkv7_backward_bf16": ((), {"r": _ACTS_BWD + " " + _GRADS}),
    "vrwkv_wkv7_backward_state_bf16": ((), {"r": _ACTS_BWD, "o": "s0 ds_final ds0", "r2": _GRADS}),
    "vrwkv_wkv7_backward_packed_bf16": ((), {"r": _ACTS_BWD, "b": "chunk_reset", "r2": _GRADS}),
    "vrwkv_wkv7_backward_segments_bf16": ((1,), {"r": _ACTS_BWD, "o": "ds_in ds_out", "r2": _GRADS}),
}


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_return_codes_of_every_launch_entry(emu_lib, name):
    """The argument checks in their order -- sizes, NULL pointers, (segments) nseg, alignment -- of all seven entries.  No kernel runs: every
    call here fails a check, so one aligned dummy buffer stands for every tensor."""
    extra, groups = ENTRIES[name]
    kinds = [kind[0] for kind, names in groups.items() for _ in names.split()]
    buf = torch.zeros(64, dtype=torch.uint8)
    good = buf.data_ptr() + (-buf.data_ptr()) % 16
    fn = _entry(emu_lib, name, 3 + len(extra), len(kinds))
    B, T, H = 2, 32, 2

    def call(B=B, T=T, extra=extra, ptrs=None):
        return fn(B, T, H, *extra, *[VP(p) for p in (ptrs or [good] * len(kinds))], None)

    def with_(ptrs, i, value):
        return [value if j == i else p for j, p in enumerate(ptrs or [good] * len(kinds))]

    before = emu_lib.vrwkv_wkv7_last_variant(0), emu_lib.vrwkv_wkv7_last_variant(1)
    assert call(T=15) == ESHAPE
    assert call(B=0) == EINVAL
    required = [i for i, kd in enumerate(kinds) if kd == "r"]
    for i in required:
        assert call(ptrs=with_(None, i, 0)) == EINVAL, i
    for i, kd in enumerate(kinds):
        if kd != "b":
            assert call(ptrs=with_(None, i, good + 2)) == EALIGN, i
    assert call(T=15, ptrs=with_(None, required[0], 0)) == ESHAPE                       # the sizes come before the pointers
    assert call(ptrs=with_(with_(None, required[0], good + 2), required[-1], 0)) == EINVAL      # NULL comes before alignment
    if extra:
        for nseg in (0, T // 16 + 1):
            assert call(extra=(nseg,)) == ESHAPE
            assert call(extra=(nseg,), ptrs=with_(None, required[0], good + 2)) == ESHAPE       # nseg comes before alignment
        assert call(extra=(0,), ptrs=with_(None, required[0], 0)) == EINVAL                    # and after NULL
    if name == "vrwkv_wkv7_forward_packed_bf16":
        for i in (kinds.index("o"), kinds.index("o") + 1):                                  # s_ckpt and sa go together
            assert call(ptrs=with_(None, i, 0)) == EINVAL
    if name == "vrwkv_wkv7_backward_packed_bf16":
        assert emu_lib.vrwkv_wkv7_set_backward_variant(5) == 0
        try:
            assert call() == ESHAPE                                                         # wkv7_bwd_v5.h has no resets
        finally:
            emu_lib.vrwkv_wkv7_set_backward_variant(-1)
    assert before == (emu_lib.vrwkv_wkv7_last_variant(0), emu_lib.vrwkv_wkv7_last_variant(1))     # nothing was launched


def test_wrappers_refuse_a_tensor_on_another_device():
    """Every wrapper checks that all activations live on w's device before it loads the library or launches."""
    from visualrwkv_amd import wkv7
    B, T, H = 1, 16, 1
    w, q, k, v, z, a, dy = make_inputs(B, T, H, seed=4)
    s, sa = torch.zeros(B, H, T // 16, 64, 64), torch.zeros(B, T, H, 64)
    lay = wkv7.PackedLayout([[T]], T)
    away = q.to("meta")
    for call in (lambda: wkv7.wkv7_forward_state(w, away, k, v, z, a),
                 lambda: wkv7.wkv7_backward_state(w, away, k, v, z, a, dy, s, sa),
                 lambda: wkv7.wkv7_forward_packed(w, away, k, v, z, a, lay),
                 lambda: wkv7.wkv7_backward_packed(w, away, k, v, z, a, dy, s, sa, lay),
                 lambda: wkv7.wkv7_backward_tparallel(w, away, k, v, z, a, dy, s, sa, 1)):
        with pytest.raises(ValueError, match="same device"):
            call()
