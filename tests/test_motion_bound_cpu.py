"""What keeps tests/test_gpu_motion_per_element.py honest, checked where no
kernel runs (tests/motion_oracle.py only): 64 x cin weights, 96 queries (three
workgroups), cin in {49, 196, 324}, both KSPLIT forms.

An arithmetic that does what the fused kernel's comments say (``emulate``,
``emulate_six``) stays inside its per-element bound on the ``unit`` and the
``wide`` data; each flawed arithmetic exceeds the bound somewhere on ``wide``;
flushed f16 subnormals stay under the 1e-4 max-norm tolerance on ``unit`` data,
which is why tests/test_gpu_motion.py could not see them.

Largest fraction of the bound used by the emulations (recorded, not asserted
beyond <= 1): pair 0.051 on unit and 0.66 on wide data; bf16 fallback 0.026 on
unit, 0.028 on wide.
"""
from __future__ import annotations

import numpy as np
import pytest

import motion_oracle as mo

COUT, NQ = 64, 96
CINS = (49, 196, 324)


def _case(kind, cin):
    return mo.inputs(kind, 7000 + cin, COUT, cin, NQ)


@pytest.mark.parametrize("ksplit", [1, 2])
@pytest.mark.parametrize("cin", CINS)
@pytest.mark.parametrize("kind", ["unit", "wide"])
def test_emulations_stay_inside_their_bounds(kind, cin, ksplit):
    w, bias, x = _case(kind, cin)
    t = mo.terms(w, x)
    for b in (bias, None):
        got, fell = mo.emulate(w, x, b, ksplit)
        assert not fell.any()
        fp = mo.fraction(got, mo.reference(t, b), mo.bound_pair(t, b, ksplit))
        f6 = mo.fraction(mo.emulate_six(w, x, b, ksplit), mo.reference(t, b), mo.bound_six(t, b, ksplit))
        print(f"{kind} cin {cin} KSPLIT {ksplit} bias {b is not None}: pair uses {fp:.4f}, "
              f"bf16 fallback {f6:.4f} of the bound")
        assert fp <= 1.0 and f6 <= 1.0


@pytest.mark.parametrize("ksplit", [1, 2])
@pytest.mark.parametrize("cin", CINS)
@pytest.mark.parametrize("flaw", ["flush", "drop", "scale", "unpadded"])
def test_every_flaw_exceeds_the_bound_on_wide_data(flaw, cin, ksplit):
    assert cin % 16 != 0
    w, bias, x = _case("wide", cin)
    t = mo.terms(w, x)
    got, _ = mo.emulate(w, x, bias, ksplit, flaw)
    f = mo.fraction(got, mo.reference(t, bias), mo.bound_pair(t, bias, ksplit))
    print(f"wide cin {cin} KSPLIT {ksplit} {flaw}: {f:.3g} of the bound")
    assert f > 1.0


@pytest.mark.parametrize("ksplit", [1, 2])
@pytest.mark.parametrize("cin", CINS)
def test_fallback_data_and_no_fallback_flaw(cin, ksplit):
    """``wide`` with one weight of 1e5: every workgroup falls back and meets the
    fallback bound; an arithmetic that keeps the pair result does not."""
    w, bias, x = _case("wide", cin)
    w, c = mo.with_overflowing_weight(w, x)
    for a in (w, x):
        assert np.abs(a[a != 0]).min() >= 2.0 ** -100
    t = mo.terms(w, x)
    got, fell = mo.emulate(w, x, bias, ksplit)
    assert fell.all()
    f = mo.fraction(got, mo.reference(t, bias), mo.bound_six(t, bias, ksplit))
    print(f"fallback cin {cin} KSPLIT {ksplit} (1e5 on channel {c}): {f:.4f} of the bound")
    assert f <= 1.0
    bad, _ = mo.emulate(w, x, bias, ksplit, "no_fallback")
    assert mo.fraction(bad, mo.reference(t, bias), mo.bound_six(t, bias, ksplit)) > 1.0
    assert mo.fraction(bad, mo.reference(t, bias), mo.bound_pair(t, bias, ksplit)) > 1.0


@pytest.mark.parametrize("cin", CINS)
def test_unit_data_cannot_see_a_flush(cin):
    w, bias, x = _case("unit", cin)
    t = mo.terms(w, x)
    ref = mo.reference(t, bias)
    got, _ = mo.emulate(w, x, bias, 2, "flush")
    err = np.abs(got - ref).max() / np.abs(ref).max()
    f = mo.fraction(got, ref, mo.bound_pair(t, bias, 2))
    print(f"unit cin {cin} flush: {err:.2e} of max|ref|, {f:.1f} of the per-element bound")
    assert err < 1e-4


@pytest.mark.parametrize("cin", CINS)
def test_zero_magnitude_is_exactly_zero(cin):
    w, _, x = _case("wide", cin)
    t = mo.terms(w, x)
    zero = t["M0"] == 0
    assert zero[:, mo.ZERO_Q].all() and not zero.all()
    for ksplit in (1, 2):
        assert (mo.emulate(w, x, None, ksplit)[0][zero] == 0).all()
        assert (mo.emulate_six(w, x, None, ksplit)[zero] == 0).all()
    assert (mo.bound_pair(t, None, 2)[zero] == 0).all()


def test_wide_data_is_what_it_says():
    w, bias, x = _case("wide", 324)
    assert np.abs(x).max() == np.float32(mo.X_TOP) < mo.F16_LIMIT
    with np.errstate(over="ignore"):
        assert np.float16(mo.X_TOP) == np.float16(65504) and np.isinf(np.float16(mo.F16_LIMIT))
    assert 0.08 < (x == 0).mean() < 0.14
    tiny = np.abs(x[:, np.arange(NQ) % mo.QB < 8]).max()
    assert tiny < 2.0 ** -20 * 2.0 ** 13 and np.abs(w[:8]).max() < 2.0 ** -20 * 2.0 ** 5
    for a in (w, x):       # operands on both sides of float16's normal range and of 2^-25
        m = np.abs(a[a != 0])
        assert (m < 2.0 ** -25).mean() > 0.1 and (m >= mo.F16_MIN_NORMAL).mean() > 0.1
        assert ((m >= 2.0 ** -25) & (m < mo.F16_MIN_NORMAL)).mean() > 0.1


def test_restatements():
    assert [mo.cin_of(*c) for c in mo.CONFIGS] == [324, 196, 162, 49]
    assert [mo.cin_pad(c) // 16 for c in (324, 196, 162, 49)] == [21, 13, 11, 4]
    assert mo.ksplit_of(2, 9 * 13) == 2 and mo.ksplit_of(3, 53 * 53) == 1
    assert mo.ksplit_of(1, 256 * 32) == 2 and mo.ksplit_of(1, 256 * 32 + 1) == 1
    assert mo.gamma_pair(324, 2, True) == 324 + 4
    a = np.array([0.0, 2.0 ** -40, 2.0 ** -14, 1.0])
    assert list(mo._d(a)) == [0.0, 2.0 ** -25, 2.0 ** -25, 2.0 ** -11]
    assert list(mo._e(a)) == [0.0, 2.0 ** -36, 2.0 ** -36, 2.0 ** -22]
    hi, mid, lo = mo.split_bf16(np.array([np.pi, -1e-30, 65519.0], dtype=np.float32))
    assert np.array_equal((hi.astype(np.float64) + mid + lo).astype(np.float32),
                          np.array([np.pi, -1e-30, 65519.0], dtype=np.float32))
