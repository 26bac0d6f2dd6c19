"""The drop-in claim itself: the reference's own `src/model.py` -- its WindBackstepping, RUN_CUDA_RWKV7g,
RWKV_Tmix_x070, RWKV_CMix_x070, Block and RWKV, unchanged -- runs on top of the operator this package registers when the reference's import-time
JIT build of its CUDA sources is replaced by `import visualrwkv_amd.wkv7`, takes this package's state dict and agrees with this package's mirror
of the same classes.  tests/golden/make_golden_dropin.py ran the reference's stack that way and recorded, per tensor, shape, norm and SHA-256 of
its state dict and results in tests/golden/dropin_ref.json; here the mirror builds the same state dict, runs on the same operator (the op's CPU
key) and must reproduce them bit for bit."""
import json
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def test_reference_model_py_runs_on_this_operator():
    from types import SimpleNamespace
    from tests.golden.make_golden_dropin import init_weights, inputs, record, run
    import visualrwkv_amd.wkv7  # noqa: F401   registers torch.ops.wind_backstepping
    from visualrwkv_amd import rwkv7 as mine
    with open(os.path.join(HERE, "golden", "dropin_ref.json")) as f:
        rec = json.load(f)
    torch.manual_seed(3)
    m_model = init_weights(mine.RWKV(SimpleNamespace(**rec["args"])))
    # the reference's state dict: same parameter names and shapes, and the same bf16 values
    state = {k: record(v) for k, v in m_model.state_dict().items()}
    assert sorted(state) == sorted(rec["state"])
    assert [k for k in state if state[k] != rec["state"][k]] == []
    x, gout = inputs()
    lm, xm, gm = run(m_model, x, gout)
    assert tuple(lm.shape) == (2, 37, 512) == tuple(rec["logits"]["shape"]) and torch.isfinite(lm.float()).all() and torch.isfinite(xm.float()).all()
    assert sorted(gm) == sorted(rec["grads"]) and len(gm) >= 40
    rel = lambda t, r: abs(float(t.double().norm()) - r["norm"]) / (r["norm"] + 1e-30)      # diagnostics only
    bad = {n: rel(t, r) for n, t, r in [("logits", lm, rec["logits"]), ("dx", xm, rec["dx"])] + [(k, gm[k], rec["grads"][k]) for k in sorted(gm)]
           if record(t) != r}
    # both stacks call the SAME operator (the host-core kernels) with the same eager bf16 arithmetic around it: bit-identical
    assert bad == {}, f"differ from the reference's results (relative difference of the norms): {bad}"
