"""The two comparisons that tests/test_glue_shapes.py and tests/test_ln_shapes.py share, each against a module's own bounds: a bf16
activation against the fp64 reference rounded once (act), one fp32 vector per channel against the fp64 reference (par).  Every figure
is recorded in `worst` per backend; VRWKV_TEST_NOTES=1 prints it with the running worst."""
import torch

from tests.parity import NOTES, bf16_close, group_bias


class Checks:
    def __init__(self, label, flip, perr, tol=1e-3):
        """flip, perr: {backend name: bound}."""
        self.label, self.flip, self.perr, self.tol = label, flip, perr, tol
        self.worst = {b: {"flip": (0.0, ""), "perr": (0.0, "")} for b in flip}

    def note(self, be, kind, val, name):
        if val > self.worst[be.name][kind][0]:
            self.worst[be.name][kind] = (val, name)
        if NOTES:
            w = self.worst[be.name]
            print(f"[{self.label}] {be.name} {name}: {kind} {val:.3e}   (worst so far: flip {w['flip'][0]:.3e} {w['flip'][1]}, "
                  f"perr {w['perr'][0]:.3e} {w['perr'][1]})")

    def act(self, be, got, ref, name, guard=True):
        """An activation or activation gradient (rows without the guard) against the fp64 reference rounded once to bf16."""
        x = (got[:-1] if guard else got).reshape(-1)
        rr = ref.detach().reshape(-1).float().bfloat16()
        assert x.shape == rr.shape, (name, x.shape, rr.shape)
        self.note(be, "flip", float((x.float() != rr.float()).float().mean()), name)
        bf16_close(x, ref, name, tol=self.tol, max_flip=self.flip[be.name])

    def par(self, be, got, ref, name):
        """One fp32 vector (C) against the fp64 reference."""
        g, r = got.double().cpu(), ref.detach().double().cpu()
        rms = float(r.pow(2).mean().sqrt())
        if rms == 0.0:
            assert not bool(g.any()), f"{name}: the reference is zero"
            return
        err = float((g - r).abs().max()) / rms
        self.note(be, "perr", err, name)
        c = int((g - r).abs().argmax())
        assert err < self.perr[be.name], (f"{name}: max_c |got - ref| / rms(ref) = {err:.3e} at channel {c} "
                                          f"(got {float(g[c]):.6e}, ref {float(r[c]):.6e})")
        group_bias(g, r, name)
