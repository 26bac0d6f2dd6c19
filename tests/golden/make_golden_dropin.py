"""Generate tests/golden/dropin_ref.json for tests/test_dropin_reference_cpu.py: imports the REFERENCE's own
VisualRWKV-v7/v7.00/src/model.py with `import visualrwkv_amd.wkv7` in place of its JIT build of the CUDA operator -- exactly the patch
INTEGRATION.md section 1 describes -- and runs the reference's RWKV (its WindBackstepping / RUN_CUDA_RWKV7g / RWKV_Tmix_x070 / RWKV_CMix_x070 / Block /
RWKV classes, its code, unchanged) on top of torch.ops.wind_backstepping as this package registers it (CPU key: libvisualrwkv_host.so).
Records, per tensor, shape, L2 norm and SHA-256 of the bf16 bytes of the reference model's state dict (its own initialisers, seeded) and of
what the reference's stack computed from it (logits, input gradient, parameter gradients) on seeded inputs; the test rebuilds the same state
dict with this package's mirror of the same classes, checks it against the record, runs the mirror and compares bit for bit.
Stand-ins only for third-party packages that are not installed (pytorch_lightning, deepspeed, timm behind src.vision); nothing of the
reference's source is stored -- only tensors.

    python tests/golden/make_golden_dropin.py <reference checkout>/VisualRWKV-v7/v7.00
"""
import hashlib
import json
import os
import sys
import types
from types import SimpleNamespace

import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

ARGS = dict(n_embd=128, dim_att=128, n_layer=2, head_size_a=64, head_size_divisor=8, vocab_size=512, dropout=0, grad_cp=0,
            ctx_len=64, load_model="", my_testing="x070", dim_ffn=512, fused=False)
T = 37                                                # not a multiple of 16: the reference left-pads with emb(STOP_TOKEN_INDEX) (src/model.py:286-312)


def inputs():
    x = (torch.randn(2, T, 128, generator=torch.Generator().manual_seed(9)) * 0.5).bfloat16()
    gout = (torch.randn(2, T, 512, generator=torch.Generator().manual_seed(10)) * 0.1).bfloat16()
    return x, gout


def init_weights(model):
    """After the model's own (seeded) initialisers: the reference zero-initialises several projections -- make every path live."""
    with torch.no_grad():
        g = torch.Generator().manual_seed(5)
        for p in model.parameters():
            if float(p.abs().sum()) == 0.0:
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    return model.bfloat16()


def record(t):
    """Shape, L2 norm and SHA-256 of the bytes of a bf16 tensor."""
    t = t.detach().contiguous()
    return {"shape": list(t.shape), "norm": float(t.double().norm()), "sha256": hashlib.sha256(t.view(torch.int16).numpy().tobytes()).hexdigest()}


def run(model, x, gout):
    """logits, d(input), {name: d(parameter)} of one forward + backward, on ONE host thread: how the bf16 weight-gradient
    reductions are split between threads changes their rounding (up to 1e-2 relative between 1 and 16 threads)."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        xi = x.clone().requires_grad_(True)
        logits = model(xi)
        logits.backward(gout)
    finally:
        torch.set_num_threads(threads)
    return logits.detach(), xi.grad, {n: p.grad for n, p in model.named_parameters() if p.grad is not None}


def main(ref_dir):
    sys.path.insert(0, ref_dir)
    pl = types.ModuleType("pytorch_lightning")
    pl.LightningModule = nn.Module
    pl.__version__ = "1.9.5"
    plu = types.ModuleType("pytorch_lightning.utilities")
    plu.rank_zero_info = lambda *a, **k: None
    plu.rank_zero_warn = lambda *a, **k: None
    pls = types.ModuleType("pytorch_lightning.strategies")
    pls.DeepSpeedStrategy = type("DeepSpeedStrategy", (), {})
    sys.modules.update({"pytorch_lightning": pl, "pytorch_lightning.utilities": plu, "pytorch_lightning.strategies": pls})
    vis = types.ModuleType("src.vision")
    vis.SamDinoSigLIPViTBackbone = type("SamDinoSigLIPViTBackbone", (nn.Module,), {})
    sys.modules["src.vision"] = vis
    os.environ["RWKV_JIT_ON"] = "0"
    os.environ["RWKV_HEAD_SIZE_A"] = "64"
    import torch.utils.cpp_extension as ce
    ce.load = lambda *a, **k: None                    # the reference's import-time JIT build of cuda/wkv7_cuda.cu ...
    import visualrwkv_amd.wkv7 as vw                  # ... replaced by this import: registers torch.ops.wind_backstepping
    from src import model as ref                      # the reference module itself, unchanged

    assert ref.WindBackstepping is not vw.WindBackstepping and ref.RUN_CUDA_RWKV7g is not vw.RUN_CUDA_RWKV7g      # the reference's own autograd surface drives the op
    torch.manual_seed(3)
    r_model = init_weights(ref.RWKV(SimpleNamespace(**ARGS)))
    x, gout = inputs()
    logits, dx, grads = run(r_model, x, gout)
    assert torch.isfinite(logits.float()).all() and torch.isfinite(dx.float()).all()
    out = os.path.join(HERE, "dropin_ref.json")
    with open(out, "w") as f:
        json.dump({"args": ARGS, "state": {k: record(v) for k, v in r_model.state_dict().items()}, "logits": record(logits), "dx": record(dx),
                   "grads": {k: record(v) for k, v in grads.items()}}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(out, tuple(logits.shape), len(grads), "parameter gradients")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
