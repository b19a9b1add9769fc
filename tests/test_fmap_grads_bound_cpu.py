"""What keeps tests/test_gpu_fmap_grads_per_element.py honest, checked where no
kernel runs (tests/fmap_grads_oracle.py only).

For every ``wide`` case the GPU file uses: an arithmetic that meets the stated
contract of the f16-pair form exactly (``emulate``) uses at most half of the
per-element bound; each flawed arithmetic exceeds it somewhere; the data does
reach the float16 subnormal range, the floor-mode remainders and all-zero
outputs.  For every ``uniform`` case (the data the max-norm tests feed) the
flushed-subnormal arithmetic stays inside the bound: that data cannot see it.

``floor_mask`` can only show where a pooled level leaves a remainder row or
column: of the five shapes only (2, 64, 23, 37, 3).  Elsewhere the flawed fold
is the fold, which is asserted instead.
"""
from __future__ import annotations

import numpy as np
import pytest

import fmap_grads_oracle as fo

IDS = ["x".join(map(str, s)) for s in fo.SHAPES]


def _fractions(c, got, slot_max=None):
    """The largest |got - ref| / bound_pair of each output."""
    ref = fo.reference(c)
    out = []
    for name, g, f, kt in (("df1", got[0], c.f2, True), ("df2", got[1], c.f1, False)):
        t = ref[name]
        S = fo.k_chunks(c.B, c.D, c.H, c.W, kt)
        b = fo.bound_pair(t, f, c.gmax if slot_max is None else slot_max, c.div, c.L, S)
        out.append(fo.fraction(np.abs(g - t["ref"]), b))
    return out


@pytest.mark.parametrize("shape", fo.SHAPES, ids=IDS)
def test_wide_emulation_within_half_and_every_flaw_exceeds(shape):
    c = fo.shape_case(shape, "wide")
    for factor in (1.0, 3000.0):
        fr = _fractions(c, fo.emulate(c, slot_max=c.gmax * factor), c.gmax * factor)
        print(f"{shape} wide x{factor:g}: emulation uses {fr[0]:.3f} / {fr[1]:.3f} of the bound")
        assert max(fr) <= 0.5
    has_remainder = bool(fo.remainder_levels(c.H, c.W, c.L))
    clean = fo.emulate(c)
    for flaw in fo.FLAWS:
        got = fo.emulate(c, flaw)
        if flaw == "floor_mask" and not has_remainder:
            assert all(np.array_equal(a, b) for a, b in zip(got, clean))
            continue
        fr = _fractions(c, got)
        print(f"{shape} wide {flaw}: {fr[0]:.1f} / {fr[1]:.1f} of the bound")
        # dF1 sees every flaw (a query's row of dV has one scale); a dF2 element sums
        # over queries of every scale, where the large ones can hide a flush
        assert fr[0] > 1.0 and (flaw == "flush" or fr[1] > 1.0), flaw


def test_some_shape_has_remainders_at_two_levels():
    assert [s for s in fo.SHAPES if len(fo.remainder_levels(*s[2:])) >= 2] == [fo.EDGE_SHAPE]


@pytest.mark.parametrize("shape", fo.SHAPES, ids=IDS)
def test_wide_data_reaches_the_edges(shape):
    c = fo.shape_case(shape, "wide")
    B, N = c.B, c.N
    # scaled operands inside the float16 subnormal range, for a tight and a loose bound
    for factor in (1.0, 3000.0):
        sf, sv = fo.subnormal_share(c, c.gmax * factor)
        print(f"{shape} x{factor:g}: f16-subnormal parts in {sf:.3f} of the fmap and {sv:.3f} of "
              f"the dV operand elements")
        assert sf >= 0.005 and sv >= 0.1
    # gradient on every level, and in every remainder row and column
    for g in c.G:
        assert (g != 0).any()
    for lvl, odd_h, odd_w in fo.remainder_levels(c.H, c.W, c.L):
        g = c.G[lvl]
        for b in range(B):
            if odd_h:
                assert (g[b * N:(b + 1) * N, -1, :] != 0).any(), (lvl, b)
            if odd_w:
                assert (g[b * N:(b + 1) * N, :, -1] != 0).any(), (lvl, b)
    # dead queries (zero dF1 columns), zero channels (zero rows), and live elements beside them
    for t in fo.reference(c).values():
        assert (t["A"] == 0).any() and (t["A"] > 0).any()
        assert (t["ref"][t["A"] == 0] == 0).all()
    dead = np.arange(B * N) % 11 == 0
    assert all(not g[dead].any() for g in c.G)
    assert (fo.reference(c)["df1"]["A"].transpose(0, 2, 3, 1).reshape(B * N, -1)[dead] == 0).all()
    # sparsity: from one cell per level (a level-l cell folds onto 4^l targets) to about 100
    n = fo.reference(c)["df1"]["n"]
    assert n[n > 0].min() <= sum(4 ** lvl for lvl in range(c.L)) and n.max() >= min(100, N // 2)


@pytest.mark.parametrize("shape", fo.SHAPES, ids=IDS)
def test_uniform_data_cannot_see_a_flush(shape):
    """On N(0, 1) pyramids every element's low part is a float16 normal or its
    loss is far below the bound: reading subnormals as zero stays inside."""
    c = fo.shape_case(shape, "uniform")
    fr = _fractions(c, fo.emulate(c, "flush"))
    print(f"{shape} uniform flush: {fr[0]:.3f} / {fr[1]:.3f} of the bound")
    assert max(fr) <= 1.0
    assert max(_fractions(c, fo.emulate(c))) <= 0.5


def test_scale_restatement():
    """scale_for: |m 2^s| < 2^14 <= |2 m 2^s| inside the clamp; the clamp; zero."""
    m = np.array([1.0, 0.99, 2.0 ** -20, 3.0e38, 1e-45, 2.0 ** -112, 0.0], dtype=np.float32)
    s = fo.scale_for(m)
    assert list(s) == [13, 14, 33, -114, 125, 125, 0]
    x = np.ldexp(m[:4].astype(np.float64), s[:4])
    assert (x < 2.0 ** 14).all() and (2 * x >= 2.0 ** 14).all()
    assert fo.bv_of(1.0, 4.0) == 2.0 ** -1          # 1.34 / 4 = 0.335 < 2^-1
    assert [fo.k_chunks(*s[:4], kt) for s in fo.SHAPES for kt in (True, False)] == \
        [1, 1, 4, 2, 9, 7, 4, 3, 9, 8]
