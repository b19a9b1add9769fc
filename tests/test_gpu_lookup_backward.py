"""GPU: the lookup backward, the pyramid fold and the NCHW pool, cell by cell
against the float64 oracle.

``dxr_corr_lookup_backward`` (and its ``_multi`` / ``_multi_bound`` forms) is
compared where it writes: every cell of every level of the gradient pyramid
against ``oracle.corr_lookup_backward`` (pinned at these very inputs by
tests/test_oracle_golden.py::test_lookup_backward_oracle_is_adjoint_of_lookup),
over every radius 0..8, windows off the level, integer, far and non-finite
coordinates, row-major levels, a 1 x 1 level, accumulation into a non-zero
pyramid and non-finite output gradients.  Cells the lookup does not tap must
keep their bits, and nothing but real cells may be written (page padding and a
guard behind the buffer included).  ``dxr_pyramid_backward`` (the dV fold, the
reference of tests/test_gpu_backward.py) and ``dxr_avg_pool2x2`` are checked
the same way.

The bounds are derived from the arithmetic (see each test), not measured.
"""
from __future__ import annotations

import ctypes
from functools import lru_cache

import numpy as np
import pytest
import torch

import datagen as dg
import oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 4096          # floats behind the pyramid, and behind the pool's output
SENTINEL = 1.5        # finite: the kernel adds, a NaN would hide a write


@pytest.fixture(scope="module")
def dx():
    import dexiraft_amd
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    dexiraft_amd.load_native()
    return dexiraft_amd


def _nat():
    from dexiraft_amd import _native
    return _native


def _t(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# --------------------------------------------------------------------------- cases
# B = 2, 18 x 26: N = 468 = 14 x 32 + 20 = 29 x 16 + 4 queries (a partial query
# block at both workgroup sizes); level widths 26, 13, 6, 3 against tile widths
# 16, 8, 4, 2, so a vector straddles the right edge on every level (the 4-, 4-,
# 4- and 2-wide column forms).  Levels >= 4 are row-major (the 1-wide form).
def _case(B=2, H=18, W=26, L=4, r=(4,), sets=(("uniform", 8.0),), entries=("single",),
          poke=False):
    return dict(B=B, H=H, W=W, L=L, r=r, sets=sets, entries=entries, poke=poke)


CASES = {f"r{k}": _case(r=(k,)) for k in range(9)}
CASES.update({
    "integer": _case(r=(4,), sets=(("integer", 4.0),)),        # zero second-tap weights
    "integer_r5": _case(r=(5,), sets=(("integer", 4.0),)),
    "far": _case(r=(1,), sets=(("far", 4.0),)),
    # both radii: the two workgroup sizes build their tap tables in different code
    "nonfinite_coords": _case(r=(4, 6), sets=(("normal", 4.0),), poke=True),
    "levels1": _case(B=1, H=9, W=13, L=1, r=(4,), sets=(("normal", 3.0),)),
    "levels2": _case(B=1, H=9, W=13, L=2, r=(4,), sets=(("normal", 3.0),)),
    "levels3": _case(B=1, H=9, W=13, L=3, r=(2,), sets=(("normal", 3.0),)),
    "levels5": _case(B=1, H=32, W=34, L=5, r=(2,), sets=(("uniform", 30.0),)),
    # level 5 is 1 x 1: the reference coordinates there are NaN (divide by W_l - 1)
    "levels6_1x1": _case(B=1, H=32, W=34, L=6, r=(2,), sets=(("uniform", 30.0),)),
    "multi3": _case(r=(4,), sets=tuple(("normal", s) for s in (3.0, 4.0, 5.0)),
                    entries=("multi", "multi_bound")),
    "multi16": _case(B=1, r=(3,), sets=tuple(("normal", 2.0 + 0.25 * k) for k in range(16)),
                     entries=("multi",)),                      # BW_MAX_SETS
})
CASE_RADII = [(cid, r) for cid, c in CASES.items() for r in c["r"]]
RUNS = [(cid, r, e) for cid, c in CASES.items() for r in c["r"] for e in c["entries"]]


def level_shapes(H: int, W: int, L: int) -> list[tuple[int, int]]:
    return [(H >> lvl, W >> lvl) for lvl in range(L)]


def poke_nonfinite(c: np.ndarray) -> np.ndarray:
    """NaN, +-inf, huge and far (-40: off levels 0-2) coordinates of a B = 2 set."""
    c[0, 0, 3, 5] = np.nan
    c[0, 1, 7, 7] = np.inf
    c[0, 0, 0, 0] = -np.inf
    c[0, 1, 2, 2] = 3e9
    c[1, :, 10, 2:24:3] = -40
    return c


def _seed(cid: str) -> int:
    return 2000 + 64 * list(CASES).index(cid)


@lru_cache(maxsize=None)
def case_inputs(cid: str, r: int):
    """(B, H, W, L, coords list, grad_out list) of a case: read-only arrays."""
    c = CASES[cid]
    B, H, W, L = c["B"], c["H"], c["W"], c["L"]
    K = L * (2 * r + 1) ** 2
    cs, gs = [], []
    for k, (mode, scale) in enumerate(c["sets"]):
        co = dg.coords(_seed(cid) + k, B, H, W, mode, scale)
        if c["poke"]:
            poke_nonfinite(co)
        go = dg.fmap(_seed(cid) + 20 + k, B, K, H, W, "normal")
        co.flags.writeable = go.flags.writeable = False
        cs.append(co)
        gs.append(go)
    return B, H, W, L, cs, gs


def oracle_grads(shapes, cs, gs, r):
    """(ref, M): the oracle's gradient levels summed over the sets, and the same
    of |grad_out| (the magnitude every bound is relative to)."""
    ref = [np.zeros((cs[0].shape[0] * cs[0].shape[2] * cs[0].shape[3],) + s) for s in shapes]
    mag = [np.zeros_like(a) for a in ref]
    with np.errstate(invalid="ignore"):
        for c, g in zip(cs, gs):
            for a, x in zip(ref, oracle.corr_lookup_backward(shapes, c, r, g)):
                a += x
            for a, x in zip(mag, oracle.corr_lookup_backward(shapes, c, r, np.abs(g))):
                a += x
    for a in ref + mag:
        a.flags.writeable = False
    return ref, mag


@lru_cache(maxsize=None)
def case_reference(cid: str, r: int):
    B, H, W, L, cs, gs = case_inputs(cid, r)
    return oracle_grads(level_shapes(H, W, L), cs, gs, r)


def check_non_vacuous(cid: str, shapes, mag) -> None:
    """The case reaches what it is there for, under the oracle alone: every level
    that can be sampled is tapped, and level 0 has untapped cells."""
    if cid == "far":
        assert all(not m.any() for m in mag)
        return
    for (h, w), m in zip(shapes, mag):
        if h >= 2 and w >= 2:
            assert (m > 0).any(), (cid, h, w)
    assert (mag[0] == 0).any(), cid


# --------------------------------------------------------------------------- helpers
def _pack(lib, nat, levels, B, H, W, L, buf):
    for lvl, a in enumerate(levels):
        t = a if isinstance(a, torch.Tensor) else _t(np.asarray(a, dtype=np.float32))
        nat.check(lib.dxr_pyramid_pack(t.data_ptr(), B, H, W, L, lvl, buf.data_ptr(), nat.DXR_F32,
                                       nat.stream_of(buf)), "pack")
    torch.cuda.synchronize()


def _unpack(lib, nat, buf, B, H, W, L):
    out = []
    for lvl, (h, w) in enumerate(level_shapes(H, W, L)):
        t = torch.full((B * H * W, h, w), float("nan"), dtype=torch.float32, device=DEV)
        nat.check(lib.dxr_pyramid_unpack(buf.data_ptr(), nat.DXR_F32, B, H, W, L, lvl, t.data_ptr(),
                                         nat.stream_of(buf)), "unpack")
        out.append(t.cpu().numpy())
    return out


def _base_levels(seed, B, H, W, L, zero=False):
    return [np.zeros((B * H * W, h, w), np.float32) if zero else
            dg.normal(seed + lvl, B * H * W * h * w).reshape(B * H * W, h, w).astype(np.float32)
            for lvl, (h, w) in enumerate(level_shapes(H, W, L))]


def _run(B, H, W, L, r, coords_list, gout_list, entry, base_seed=7000, zero_base=False):
    """Run one entry point once over the whole list into a sentinel-filled,
    guarded buffer holding a random base pyramid.  Returns (base levels, unpacked
    levels after the call, the whole buffer, bound slots or None) after checking
    that nothing but real cells was written."""
    nat = _nat()
    lib = nat.load()
    numel = lib.dxr_pyramid_numel(B, H, W, L)
    buf = torch.full((numel + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    base = _base_levels(base_seed, B, H, W, L, zero_base)
    _pack(lib, nat, base, B, H, W, L, buf)
    before = buf.clone()
    cs = [_t(np.array(c)) for c in coords_list]     # copies: the cases' arrays are read-only
    gs = [_t(np.array(g)) for g in gout_list]
    s = nat.stream_of(buf)
    n = len(cs)
    slots = None
    if entry == "single":
        for c, g in zip(cs, gs):
            nat.check(lib.dxr_corr_lookup_backward(c.data_ptr(), g.data_ptr(), B, H, W, L, r,
                                                   buf.data_ptr(), nat.DXR_F32, s), entry)
    else:
        cp = (ctypes.c_void_p * n)(*[c.data_ptr() for c in cs])
        gp = (ctypes.c_void_p * n)(*[g.data_ptr() for g in gs])
        if entry == "multi":
            nat.check(lib.dxr_corr_lookup_backward_multi(cp, gp, n, B, H, W, L, r, buf.data_ptr(),
                                                         nat.DXR_F32, s), entry)
        else:
            assert entry == "multi_bound"
            nsl = lib.dxr_lookup_backward_bound_slots(B, H, W, L, r)
            assert nsl > 0
            slots = torch.zeros(nsl, dtype=torch.float32, device=DEV)
            nat.check(lib.dxr_corr_lookup_backward_multi_bound(cp, gp, n, B, H, W, L, r,
                                                               buf.data_ptr(), nat.DXR_F32,
                                                               slots.data_ptr(), s), entry)
    torch.cuda.synchronize()
    after = _unpack(lib, nat, buf, B, H, W, L)
    # nothing but real cells was written: with the real cells zeroed on both
    # sides, the buffers (page padding and guard included) are the same bits
    zeros = [torch.zeros(a.shape, dtype=torch.float32, device=DEV) for a in base]
    a0, b0 = before.clone(), buf.clone()
    _pack(lib, nat, zeros, B, H, W, L, a0)
    _pack(lib, nat, zeros, B, H, W, L, b0)
    assert torch.equal(a0, b0), "a cell outside the levels (padding or guard) was written"
    return base, after, buf, slots


def _check_levels(tag, base, after, ref, mag):
    """Per level and cell: |got - ref| <= 2^-20 M + 2^-22 |base|, and the base's
    bits where M == 0.

    The tap weights are the forward's float32 weights in the kernel and in the
    oracle.  A cell is a sum of at most 3 x 3 terms through two fma chains with
    one product-order difference per term: ~8 roundings of 2^-24 relative to M,
    doubled.  ``old + acc`` rounds once per set relative to |base| + M: the
    second term, with 16 sets in mind."""
    worst = 0.0
    for lvl, (b, a, rf, m) in enumerate(zip(base, after, ref, mag)):
        assert a.shape == rf.shape
        got = a.astype(np.float64) - b.astype(np.float64)
        fin = np.isfinite(rf)
        err = np.abs(got[fin] - rf[fin])
        bound = 2.0 ** -20 * m[fin] + 2.0 ** -22 * np.abs(b[fin]).astype(np.float64)
        if err.size:
            with np.errstate(divide="ignore", invalid="ignore"):
                rel = np.where(m[fin] > 0, err / m[fin], 0.0)
                use = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
            i = int(np.argmax(use))
            print(f"{tag} level {lvl}: max |got - ref| / M {rel.max():.3e}, max err / bound "
                  f"{use[i]:.3f} at got {got[fin][i]:.9e} ref {rf[fin][i]:.9e} M {m[fin][i]:.3e} "
                  f"base {b[fin][i]:.3e}")
            worst = max(worst, float(use[i]))
            assert (err <= bound).all(), (tag, lvl)
        untouched = m == 0
        assert np.array_equal(a.view(np.int32)[untouched], b.view(np.int32)[untouched]), \
            f"{tag} level {lvl}: a cell no sample taps changed its bits"
    print(f"{tag}: max err / bound over all levels {worst:.3f}")
    return worst


# --------------------------------------------------------------------------- lookup backward
@pytest.mark.parametrize("cid,r,entry", RUNS, ids=[f"{c}-r{r}-{e}" for c, r, e in RUNS])
def test_lookup_backward_matches_oracle_per_cell(dx, cid, r, entry):
    B, H, W, L, cs, gs = case_inputs(cid, r)
    ref, mag = case_reference(cid, r)
    check_non_vacuous(cid, level_shapes(H, W, L), mag)
    base, after, buf, slots = _run(B, H, W, L, r, cs, gs, entry, base_seed=_seed(cid) + 40)
    _check_levels(f"{cid} r={r} {entry}", base, after, ref, mag)


def test_far_queries_leave_the_whole_buffer_unchanged(dx):
    """Every query far: the whole buffer (guard included) keeps its bits."""
    B, H, W, L, cs, gs = case_inputs("far", 1)
    nat = _nat()
    lib = nat.load()
    numel = lib.dxr_pyramid_numel(B, H, W, L)
    buf = torch.full((numel + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    _pack(lib, nat, _base_levels(_seed("far") + 40, B, H, W, L), B, H, W, L, buf)
    before = buf.clone()
    c, g = _t(np.array(cs[0])), _t(np.array(gs[0]))
    nat.check(lib.dxr_corr_lookup_backward(c.data_ptr(), g.data_ptr(), B, H, W, L, 1,
                                           buf.data_ptr(), nat.DXR_F32, nat.stream_of(buf)), "far")
    torch.cuda.synchronize()
    assert torch.equal(buf, before)


def test_multi_bound_equals_multi_and_bounds_the_gradient(dx):
    """multi3: the bound form writes multi's buffer bit for bit, and its slots'
    maximum is at least the largest gradient cell the oracle finds."""
    B, H, W, L, cs, gs = case_inputs("multi3", 4)
    ref, _ = case_reference("multi3", 4)
    seed = _seed("multi3") + 40
    _, _, buf_m, _ = _run(B, H, W, L, 4, cs, gs, "multi", base_seed=seed, zero_base=True)
    _, _, buf_b, slots = _run(B, H, W, L, 4, cs, gs, "multi_bound", base_seed=seed, zero_base=True)
    assert torch.equal(buf_m, buf_b)
    top = max(float(np.abs(a).max()) for a in ref)
    assert top > 0 and slots.max().item() >= top
    _, _, buf_m, _ = _run(B, H, W, L, 4, cs, gs, "multi", base_seed=seed)
    _, _, buf_b, _ = _run(B, H, W, L, 4, cs, gs, "multi_bound", base_seed=seed)
    assert torch.equal(buf_m, buf_b)


def test_nonfinite_grad_out_stays_in_its_taps(dx):
    """NaN / +inf output gradients reach exactly the cells their samples tap (the
    oracle's NaN and +-inf patterns, cell for cell); a NaN gradient of a query
    whose coordinate is NaN, or that is far, reaches nothing.  Fractional
    coordinates (every in-map tap weight non-zero) and a zero base, so that
    ``inf + base`` is not in question."""
    B, H, W, L, r = 2, 18, 26, 4, 4
    N, K1 = H * W, (2 * r + 1) ** 2
    c = poke_nonfinite(dg.coords(9100, B, H, W, "normal", 3.0))
    g = dg.fmap(9101, B, L * K1, H, W, "normal")
    poked = [(0, 9, 12), (1, 5, 20)]                 # two ordinary queries
    g[0, 40, 9, 12] = np.nan                         # level 0, centre sample
    g[1, K1 + 40, 5, 20] = np.inf                    # level 1, centre sample
    g[0, :, 3, 5] = np.nan                           # the NaN-coordinate query
    g[1, :3 * K1, 10, 5] = np.nan                    # a query at -40: far on levels 0-2
    shapes = level_shapes(H, W, L)
    ref, mag = oracle_grads(shapes, [c], [g], r)
    base, after, _, _ = _run(B, H, W, L, r, [c], [g], "single", zero_base=True)
    clean = np.ones(B * N, dtype=bool)
    for b, y, x in poked:
        clean[b * N + y * W + x] = False
    for lvl, (a, rf) in enumerate(zip(after, ref)):
        assert np.array_equal(np.isnan(a), np.isnan(rf)), lvl
        assert np.array_equal(np.isposinf(a), np.isposinf(rf)), lvl
        assert np.array_equal(np.isneginf(a), np.isneginf(rf)), lvl
        assert np.isfinite(a[clean]).all(), lvl
    assert np.isnan(after[0][0 * N + 9 * W + 12]).any()
    assert np.isposinf(after[1][1 * N + 5 * W + 20]).any()
    _check_levels("nonfinite grad_out", base, after, ref, mag)


@pytest.mark.parametrize("cid,r", [("r4", 4), ("r7", 7), ("levels5", 2)])
def test_backward_is_adjoint_of_forward_kernel(dx, cid, r):
    """<dxr_corr_lookup(P, c), g> == <P, dxr_corr_lookup_backward(c, g)> for a
    random pyramid P, summed in float64 on the host: two f32-computed sides, each
    within the per-cell bound (2^-20 of its terms' magnitudes), so 2^-19 of
    sum |out| |g|."""
    nat = _nat()
    lib = nat.load()
    B, H, W, L, cs, gs = case_inputs(cid, r)
    c, g = cs[0], gs[0]
    numel = lib.dxr_pyramid_numel(B, H, W, L)
    P = _base_levels(_seed(cid) + 50, B, H, W, L)
    pyr = torch.zeros(numel, dtype=torch.float32, device=DEV)
    _pack(lib, nat, P, B, H, W, L, pyr)
    ct = _t(np.array(c))
    out = torch.full(g.shape, float("nan"), dtype=torch.float32, device=DEV)
    nat.check(lib.dxr_corr_lookup(pyr.data_ptr(), nat.DXR_F32, B, H, W, L, r, ct.data_ptr(),
                                  out.data_ptr(), nat.stream_of(out)), "lookup")
    torch.cuda.synchronize()
    out = out.cpu().numpy().astype(np.float64)
    assert np.isfinite(out).all()
    _, G, _, _ = _run(B, H, W, L, r, [c], [g], "single", zero_base=True)
    lhs = float((out * g.astype(np.float64)).sum())
    rhs = float(sum((p.astype(np.float64) * q.astype(np.float64)).sum() for p, q in zip(P, G)))
    scale = float((np.abs(out) * np.abs(g).astype(np.float64)).sum())
    print(f"{cid}: <out, g> {lhs:.9e}  <P, G> {rhs:.9e}  |diff| / sum|out||g| "
          f"{abs(lhs - rhs) / scale:.3e}")
    assert scale > 0 and abs(lhs - rhs) <= 2.0 ** -19 * scale


# --------------------------------------------------------------------------- pyramid fold
def _fold(levels, divisor):
    """oracle.corr_pyramid_backward's fold: from the top level down,
    tot = G_l + avg_pool2x2_backward(tot), then / divisor.  float64."""
    tot = levels[-1].astype(np.float64)
    for lvl in range(len(levels) - 2, -1, -1):
        tot = levels[lvl].astype(np.float64) + oracle.avg_pool2x2_backward(tot,
                                                                           levels[lvl].shape[-2:])
    return tot / np.float64(divisor)


@pytest.mark.parametrize("shape", [(2, 18, 26, 4), (1, 9, 13, 3), (1, 17, 23, 1), (1, 32, 34, 5),
                                   (1, 32, 34, 6), (3, 8, 8, 4)])
def test_pyramid_backward_matches_float64_fold(dx, shape):
    """dV = (G_0 + (G_1 + ...) / 4) / sqrt(D) per cell against the float64 fold of
    the same levels; odd sizes leave the floor-mode remainder row / column with
    level 0's gradient only.  At most L + 1 roundings (the 1/4 factors are
    exact), L <= 6, doubled: 2^-21 of the same fold of |G|.  D = 48: a divisor
    that is no power of two (the true-division form)."""
    nat = _nat()
    lib = nat.load()
    B, H, W, L = shape
    numel = lib.dxr_pyramid_numel(B, H, W, L)
    gp = torch.zeros(numel, dtype=torch.float32, device=DEV)    # zero padding: the caller's contract
    levels = _base_levels(8000 + 10 * H + L, B, H, W, L)
    _pack(lib, nat, levels, B, H, W, L, gp)
    div = np.sqrt(np.float32(48), dtype=np.float32)
    dv = torch.full((B * H * W, H, W), float("nan"), dtype=torch.float32, device=DEV)
    nat.check(lib.dxr_pyramid_backward(gp.data_ptr(), nat.DXR_F32, B, H, W, L, float(div),
                                       dv.data_ptr(), nat.stream_of(dv)), "dxr_pyramid_backward")
    torch.cuda.synchronize()
    got = dv.cpu().numpy()
    assert np.isfinite(got).all()
    ref = _fold(levels, div)
    mag = _fold([np.abs(a) for a in levels], div)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"{shape}: max |dV - ref| / M {(err / mag).max():.3e}")
    assert (err <= 2.0 ** -21 * mag).all()


# --------------------------------------------------------------------------- NCHW pool
@pytest.mark.parametrize("shape", [(3, 9, 13), (2, 55, 128), (5, 7, 2), (1, 2, 2), (4, 6, 1)])
def test_avg_pool_nchw_matches_oracle(dx, shape):
    """dxr_avg_pool2x2 ([planes, H, W], floor mode) against oracle.avg_pool2x2 of
    the float64 input: three adds and an exact 1/4, so 2^-22 of each block's
    mean |x|.  The kernel sums in the oracle's order, so the result is also
    oracle.avg_pool2x2 of the float32 input bit for bit (as the NHWC kernel's,
    tests/test_gpu_channels_last.py): asserted too.  Nothing is written behind
    the output; W / 2 == 0 writes nothing at all."""
    nat = _nat()
    lib = nat.load()
    P, H, W = shape
    x = dg.normal(8500 + H, P * H * W).reshape(P, H, W).astype(np.float32)
    n = P * (H // 2) * (W // 2)
    out = torch.full((n + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    xt = _t(x)
    nat.check(lib.dxr_avg_pool2x2(xt.data_ptr(), out.data_ptr(), P, H, W, nat.stream_of(out)),
              "dxr_avg_pool2x2")
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    assert (res[n:] == np.float32(SENTINEL)).all(), "the pool wrote behind its output"
    if n == 0:
        return
    got = res[:n].reshape(P, H // 2, W // 2)
    ref = oracle.avg_pool2x2(x.astype(np.float64))
    mag = oracle.avg_pool2x2(np.abs(x).astype(np.float64))
    err = np.abs(got.astype(np.float64) - ref)
    print(f"{shape}: max |got - ref| / mean|x| {(err / mag).max():.3e}")
    assert (err <= 2.0 ** -22 * mag).all()
    np.testing.assert_array_equal(got, oracle.avg_pool2x2(x))
