"""Shared by tests/test_e2e_fused_cpu.py and tests/test_gpu_e2e_fused.py: the flow
criteria of the refinement loop (tests/e2e_flow.py) with INTEGRATION.md's inference
substitutions in it, and the ``record=`` callbacks that check a substitution inside
the loop, on the coordinates and states the update block produces.

Test infrastructure only; nothing here calls the package.  The callers hand in the
blocks and callables, so the same checks run on the GPU around the HIP pieces and
on the CPU around plain restatements of them, where deliberately wrong hooks show
that each check can fail (tests/test_e2e_fused_cpu.py).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import e2e_flow as ef
from conftest import GOLDEN

CONV1X1_OF_MAX = 1e-6   # lookup_conv1x1 against float64, of max|ref|
QUANTITIES = ("per_iter", "final", "up", "edge")


def golden() -> dict:
    with np.load(GOLDEN / "e2e_chairs.npz") as z:
        return {k: z[k] for k in z.files}


def quantities(flows, up=None, eflow=None) -> dict:
    """EPE (px) against the reference loop's recorded flows: every iteration's, the
    final one, the 8x upsampled flow (on the golden's every-fourth-pixel grid) and
    the edge flow.  A loop cut short has only ``per_iter``: the golden keeps the
    upsampled and the edge flow of the last iteration alone."""
    g = golden()
    q = {"per_iter": [ef.epe(fl, g["flows"][i]) for i, fl in enumerate(flows)]}
    if len(flows) == ef.E2E["iters"]:
        q["final"] = q["per_iter"][-1]
        q["up"] = ef.epe(up[:, :, ::4, ::4], g["flow_up_sub4"])
        q["edge"] = ef.epe(eflow, g["eflow"])
    return q


def flat(q: dict) -> list[tuple[str, float]]:
    out = [(f"iteration {i + 1}", v) for i, v in enumerate(q["per_iter"])]
    return out + [(k, q[k]) for k in QUANTITIES[1:] if k in q]


def show(what: str, q: dict) -> None:
    rest = ", ".join(f"{k} {q[k]:.3e}" for k in QUANTITIES[1:] if k in q)
    print(f"{what}: max over iterations {max(q['per_iter']):.3e} px" + (", " + rest if rest else ""))


def assert_f32_class(q: dict, tol: float) -> None:
    """The criteria of tests/test_e2e_flow.py::_check on ``quantities``."""
    assert all(np.isfinite(v) for _, v in flat(q)), q
    assert max(q["per_iter"]) < tol, q["per_iter"]
    if "final" in q:
        assert q["final"] < tol
        assert q["up"] < 8 * tol          # full-res flow is 8x the low-res flow
        assert q["edge"] < tol


def assert_within(what: str, q: dict, d: dict, factor: float = 2.0) -> float:
    """Every quantity of ``q`` is at most ``factor`` times the same quantity of ``d``;
    returns (and prints) the largest fraction of that margin that was used."""
    used = []
    for (name, v), (_, dv) in zip(flat(q), flat(d)):
        assert np.isfinite(v) and v <= factor * dv, (what, name, v, dv)
        used.append(v / (factor * dv))
    print(f"{what}: largest fraction of {factor:g} d used {max(used):.3f} "
          f"(final {q['per_iter'][-1]:.3e} px against d = {d['per_iter'][-1]:.3e} px)")
    return max(used)


def assert_rounding_in_play(d: dict, f32: dict) -> None:
    """Before the code under test is looked at: the emulated loop is finite and every
    quantity of it lies above the float32 loop's own error."""
    for (name, dv), (_, fv) in zip(flat(d), flat(f32)):
        assert np.isfinite(dv) and dv > fv, (name, dv, fv)


class States:
    """``record=``: keeps (net, x) of one stream at the given iterations (from 1)."""

    def __init__(self, iterations, stream="image"):
        self.iterations, self.stream, self.kept = set(iterations), stream, {}

    def __call__(self, it, stream, net, x, coords, corr):
        if stream == self.stream and it + 1 in self.iterations:
            self.kept[it + 1] = (net.clone(), x.clone())


class LookupCheck:
    """``record=``: what the loop's lookups returned, against the plain form on the
    same coordinates, at every iteration and for both streams.

    ``ref_lookup(stream, coords)`` is the float32 NCHW lookup of that stream's own
    block.  Without ``conv``: the loop's tensor (half of a batched block's output, a
    channels-last tensor, a 16-bit one) equals it, cast to ``cast`` where given, with
    ``torch.equal``.  With ``conv = (weight, bias)`` the loop's tensor is lookup +
    convc1 + ReLU: in float32 it lies within 1e-6 of max of
    ``relu(conv2d(ref.double(), ...))``; and where ``ref_fused(stream, coords)`` (the
    fused call on that stream's own block, float32 NCHW) is given it equals that,
    cast to ``cast``, with ``torch.equal``."""

    def __init__(self, ref_lookup, conv=None, ref_fused=None, cast=None, channels_last=False):
        self.ref_lookup, self.conv, self.ref_fused = ref_lookup, conv, ref_fused
        self.cast, self.channels_last = cast, channels_last
        self.calls, self.worst = 0, 0.0

    def __call__(self, it, stream, net, x, coords, corr):
        where = f"iteration {it + 1}, {stream} stream"
        self.calls += 1
        assert corr.dtype == (self.cast or torch.float32), where
        if self.channels_last:
            assert corr.is_contiguous(memory_format=torch.channels_last), where
        ref = self.ref_lookup(stream, coords)
        assert ref.dtype == torch.float32
        if self.conv is None:
            assert torch.equal(corr, ref if self.cast is None else ref.to(self.cast)), where
            return
        if self.ref_fused is not None:
            fused = self.ref_fused(stream, coords)
            assert torch.equal(corr, fused if self.cast is None else fused.to(self.cast)), where
        if self.cast is None:
            w, b = self.conv
            want = F.relu(_conv1x1_f64(ref, w, b))
            err = float((corr.double() - want).abs().max() / want.abs().max())
            self.worst = max(self.worst, err)
            assert err <= CONV1X1_OF_MAX, (where, err)


def _conv1x1_f64(corr, w, b):
    """conv2d(corr.double(), w.double(), b.double()) of a 1x1 kernel, as a matmul (no
    float64 convolution backend is needed on the GPU)."""
    w2 = w.double().reshape(w.shape[0], w.shape[1])
    return torch.einsum("oc,nchw->nohw", w2, corr.double()) + b.double()[None, :, None, None]
