"""GPU: the float16 correlation pyramid (``CorrBlock(..., pyramid_dtype=torch.float16)``,
DXR_PYR_F16 at the C-ABI).

The definition under test: every stored cell of every level is the float32
pyramid's cell for the same fmaps, rounded once to float16 with round-to-nearest-
even (overflow to +-inf, subnormals kept) — ``level.half()`` of the default
block's levels, bit for bit.  Lookups widen the cells on load and run the float32
arithmetic, so their reference is the float32 lookup of the widened pyramid, again
bit for bit.  Only test 7 (the accuracy statement) has a tolerance, and it is
derived: half a float16 ulp on top of the float32 build's bar.

Shapes are those of tests/test_gpu_f16.py, from the build's structure
(corr_build_dma_kernel: a stage = 32 channels, a unit = 2 x 128 queries x one 8x16
target tile; the epilogue stores 8 float16 cells = 16 B per lane):

  a  B=2 D=32  9x13   one K stage; 117 queries = one partial query block; ragged
                      8x16 target tiles, odd W; batch offset; level 3 is 1x1
  b  B=1 D=96  23x37  the ring fills exactly once; an odd number of 128-query
                      blocks plus tail quarter units
  c  B=1 D=256 16x24  the ring wraps; the production D
  d  B=3 D=32  48x64  (lookups only, tests/test_gpu_out16.py's case d) more than
                      1024 32-query workgroups: the multi-round lookup shape, whose
                      window vectors come by range-checked buffer loads, and the
                      512-thread form of the fused conv
  e  B=1 D=32 112x128 (one build) a 548 MB float16 pyramid: beyond the 512 MB
                      threshold at which the epilogue streams with non-temporal
                      stores instead of write-through ones
"""
from __future__ import annotations

import copy
from functools import lru_cache

import numpy as np
import pytest
import torch

import datagen as dg
import oracle
from conftest import tolerance_check

pytestmark = pytest.mark.gpu

RTOL = 1e-4           # the project's float32 build / lookup tolerance (of max |ref|)
DEV = "cuda:0"
CASES = {"a": (2, 32, 9, 13), "b": (1, 96, 23, 37), "c": (1, 256, 16, 24), "d": (3, 32, 48, 64),
         "e": (1, 32, 112, 128)}
SEEDS = {"a": 1610, "b": 1620, "c": 1630, "d": 1840, "e": 1690}
F16_MIN_NORMAL = 2.0 ** -14
F16_OVERFLOW = 65520.0    # the first float32 magnitude that rounds to float16 inf
OVERFLOW_SCALE = 60.0     # case c: float64 oracle max |cell| 1.2e5, 95,153 level-0 cells >= 65520


@pytest.fixture(scope="module")
def dx():
    import dexiraft_amd
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    dexiraft_amd.load_native()
    return dexiraft_amd


def _t(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _cl(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous(memory_format=torch.channels_last)


@lru_cache(maxsize=None)
def _fmaps16(case: str, scale: float = 1.0):
    """fnet-like fmaps x scale, rounded to float16 (numpy; test_gpu_f16's generator)."""
    B, D, H, W = CASES[case]
    s = SEEDS[case]
    f1 = (dg.fmap(s, B, D, H, W, "fnet") * np.float32(scale)).astype(np.float16)
    f2 = (dg.fmap(s + 1, B, D, H, W, "fnet") * np.float32(scale)).astype(np.float16)
    return f1, f2


@lru_cache(maxsize=None)
def _dev_fmaps(case: str, fdt: str, layout: str = "nchw", scale: float = 1.0):
    """The same values as float16 or (widened) float32 device tensors."""
    f1, f2 = (_t(x) for x in _fmaps16(case, scale))
    if fdt == "f32":
        f1, f2 = f1.float(), f2.float()
    return (f1, f2) if layout == "nchw" else (_cl(f1), _cl(f2))


@lru_cache(maxsize=None)
def _block(case: str, fdt: str, layout: str = "nchw", pyr: str = "f16", scale: float = 1.0,
           levels: int = 4, r: int = 4):
    """One block per configuration, shared by the tests (never modified)."""
    import dexiraft_amd
    f1, f2 = _dev_fmaps(case, fdt, layout, scale)
    kw = {"pyramid_dtype": torch.float16} if pyr == "f16" else {}
    return dexiraft_amd.CorrBlock(f1, f2, num_levels=levels, radius=r, **kw)


@lru_cache(maxsize=None)
def _ref64(case: str, scale: float = 1.0):
    """float64 oracle pyramid of the widened float16 fmaps (computed once)."""
    f1, f2 = _fmaps16(case, scale)
    return oracle.corr_pyramid(f1.astype(np.float32), f2.astype(np.float32), 4, np.float64)


@lru_cache(maxsize=None)
def _coords(case: str):
    B, D, H, W = CASES[case]
    return dg.coords(SEEDS[case] + 2, B, H, W, "uniform", 6.0)   # windows partly off the map


def assert_levels_are_half_of(cb16, cb32, what: str):
    """Every level of the float16-pyramid block == level.half().float() of the
    float32-pyramid block (torch.equal: no NaN occurs in these pyramids)."""
    assert cb16._buf.dtype == torch.float16 and cb32._buf.dtype == torch.float32
    assert cb16._buf.numel() == cb32._buf.numel()
    got, ref = cb16.corr_pyramid, cb32.corr_pyramid
    assert len(got) == len(ref)
    for lvl, (g, r) in enumerate(zip(got, ref)):
        assert g.dtype == torch.float32 and g.shape == r.shape
        assert not torch.isnan(r).any()
        want = r.half().float()
        if not torch.equal(g, want):
            bad = g != want
            i = tuple(int(v) for v in bad.nonzero()[0])
            raise AssertionError(f"{what} level {lvl}: {int(bad.sum())} of {bad.numel()} cells differ; "
                                 f"first at {i}: got {g[i].item()!r}, want {want[i].item()!r} "
                                 f"(float32 {r[i].item()!r})")


def _widened_f32_block(cb16):
    """A float32-pyramid block holding exactly the widened cells of ``cb16``:
    its levels packed into a zero-filled float32 paged buffer by dxr_pyramid_pack.
    The reference of every lookup test (float32 kernels, not under test here)."""
    from dexiraft_amd import _native as nat
    lib = nat.load()
    B, D, H, W = cb16._geom
    buf = torch.zeros(cb16._buf.numel(), dtype=torch.float32, device=DEV)
    for lvl, lev in enumerate(cb16.corr_pyramid):
        assert lib.dxr_pyramid_pack(lev.data_ptr(), B, H, W, cb16.num_levels, lvl, buf.data_ptr(),
                                    nat.DXR_F32, nat.stream_of(buf)) == nat.DXR_OK
    ref = copy.copy(cb16)
    ref._buf, ref._pyr_dt, ref._ref_pyramid = buf, nat.DXR_F32, None
    return ref


def assert_same_f32(got: torch.Tensor, ref: torch.Tensor, what: str):
    assert got.dtype == ref.dtype == torch.float32 and got.shape == ref.shape, what
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), f"{what}: NaN positions differ"
    assert torch.equal(torch.nan_to_num(got), torch.nan_to_num(ref)), f"{what}: values differ"


# ------------------------------------------------------- 1. build, bit equality
BUILDS = ([(c, "f16", lay) for c in "abc" for lay in ("nchw", "nhwc")]
          + [(c, "f32", lay) for c in "ac" for lay in ("nchw", "nhwc")])


@pytest.mark.parametrize("case,fdt,layout", BUILDS)
def test_pyr16_build_is_half_of_the_f32_pyramid(dx, case, fdt, layout):
    from dexiraft_amd import _native as nat
    B, D, H, W = CASES[case]
    cb16 = _block(case, fdt, layout, "f16")
    cb32 = _block(case, fdt, layout, "f32")
    assert_levels_are_half_of(cb16, cb32, f"case {case} {fdt} {layout}")
    # NCHW and channels-last fmaps of the same values: the same bits
    assert torch.equal(cb16._buf.view(torch.int16), _block(case, fdt, "nchw", "f16")._buf.view(torch.int16))
    # the library itself wrote DXR_PYR_F16 (no conversion pass in the Python layer):
    # one direct call into a NaN-prefilled buffer reproduces the block's buffer,
    # padding cells included
    lib = nat.load()
    f1, f2 = _dev_fmaps(case, fdt, layout)
    in_dt = nat.DXR_F16 if fdt == "f16" else nat.DXR_F32
    code = nat.DXR_NCHW if layout == "nchw" else nat.DXR_NHWC
    nbytes = 0 if (fdt == "f16" and layout == "nhwc") else lib.dxr_build_workspace_bytes(in_dt, B, D, H, W)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)
    buf = torch.full_like(cb16._buf, float("nan"))
    st = lib.dxr_corr_pyramid_build_ws(f1.data_ptr(), f2.data_ptr(), in_dt, code, B, D, H, W, 4,
                                       float(np.sqrt(np.float32(D))), buf.data_ptr(),
                                       nat.DXR_PYR_F16, nat.DXR_BUILD_AUTO,
                                       ws.data_ptr() if nbytes else None, nbytes, nat.stream_of(buf))
    assert st == nat.DXR_OK
    torch.cuda.synchronize()
    assert not torch.isnan(buf).any()
    assert torch.equal(buf.view(torch.int16), cb16._buf.view(torch.int16))


def test_pyr16_build_streamed_stores(dx):
    """Case e: a float16 pyramid beyond 512 MB takes the epilogue's non-temporal
    16-byte stores; the whole paged buffer, padding included, is the float32
    buffer's .half()."""
    B, D, H, W = CASES["e"]
    f1, f2 = _dev_fmaps("e", "f16")
    cb16 = dx.CorrBlock(f1, f2, pyramid_dtype=torch.float16)
    assert cb16._buf.numel() * 2 > 512 * (1 << 20)
    cb32 = dx.CorrBlock(f1, f2)
    assert not torch.isnan(cb32._buf).any()
    assert torch.equal(cb16._buf.view(torch.int16), cb32._buf.half().view(torch.int16))
    assert int((cb16._buf != 0).sum().item()) > cb16._buf.numel() // 2


# --------------------------------------------------------------- 2. fallback
@pytest.mark.parametrize("fdt,D", [("f16", 48), ("f32", 40)])
def test_pyr16_shapes_outside_the_fused_build(dx, fdt, D):
    """float16 fmaps with D % 32 != 0 are widened (the float32 pre-split build then
    stores float16 itself, D % 16 == 0); float32 fmaps with D % 16 != 0 build the
    float32 pyramid into a temporary and round it level by level.  The same
    pyramid by definition."""
    f1 = _t(dg.fmap(1650, 2, D, 9, 13, "fnet")).half()
    f2 = _t(dg.fmap(1651, 2, D, 9, 13, "fnet")).half()
    if fdt == "f32":
        f1, f2 = f1.float(), f2.float()
    cb16 = dx.CorrBlock(f1, f2, pyramid_dtype=torch.float16)
    cb32 = dx.CorrBlock(f1, f2)
    assert_levels_are_half_of(cb16, cb32, f"{fdt} D={D}")
    cl16 = dx.CorrBlock(_cl(f1), _cl(f2), pyramid_dtype=torch.float16)
    assert_levels_are_half_of(cl16, cb32, f"{fdt} D={D} channels-last")
    c = _t(dg.coords(1652, 2, 9, 13, "uniform", 6.0))
    assert_same_f32(cb16(c), _widened_f32_block(cb16)(c), f"{fdt} D={D} lookup")


# ----------------------------------------------------------------- 3. lookup
LOOKUPS = [("a", 4, 4), ("b", 4, 4), ("c", 4, 4), ("a", 3, 2), ("d", 4, 4)]


@pytest.mark.parametrize("case,r,levels", LOOKUPS)
def test_pyr16_lookup_is_the_f32_lookup_of_the_widened_pyramid(dx, case, r, levels):
    B, D, H, W = CASES[case]
    cb16 = _block(case, "f16", "nchw", "f16", 1.0, levels, r)
    assert cb16._buf.dtype == torch.float16
    c = _coords(case)
    got = cb16(_t(c))
    assert got.dtype == torch.float32 and got.is_contiguous()
    assert got.shape == (B, levels * (2 * r + 1) ** 2, H, W)
    assert_same_f32(got, _widened_f32_block(cb16)(_t(c)), f"case {case} r{r} L{levels}")
    assert torch.isfinite(got).any() and (got != 0).any()
    if case != "d":   # and against the float64 lookup of the same widened levels
        wide = [lev[:, 0].cpu().numpy().astype(np.float64) for lev in cb16.corr_pyramid]
        e = tolerance_check(got.cpu().numpy(), oracle.corr_lookup(wide, c, r), RTOL)
        print(f"case {case} r{r} L{levels}: lookup err/max vs float64 {e:.3e}")


# ------------------------------------------ 4. 16-bit outputs and the fused conv
@pytest.mark.parametrize("odt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("case,r,levels", LOOKUPS)
def test_pyr16_out16_equals_cast_of_its_f32_lookup(dx, case, r, levels, odt):
    from test_gpu_out16 import assert_bit_equal
    cb16 = _block(case, "f16", "nchw", "f16", 1.0, levels, r)
    c = _t(_coords(case))
    assert_bit_equal(cb16(c, out_dtype=odt), cb16(c), odt, f"case {case} r{r} L{levels} -> {odt}")


@pytest.mark.parametrize("case,r", [("c", 4), ("c", 3), ("b", 4), ("d", 4)])
def test_pyr16_lookup_conv1x1(dx, case, r):
    from test_gpu_out16 import assert_bit_equal
    B, D, H, W = CASES[case]
    cb16 = _block(case, "f16", "nchw", "f16", 1.0, 4, r)
    ref = _widened_f32_block(cb16)
    c = _t(dg.coords(SEEDS[case] + 3, B, H, W, "normal", 4.0))
    w, bias = dg.conv1x1_weights(3, 96, 4 * (2 * r + 1) ** 2)
    w, bias = _t(w), _t(bias)
    got = cb16.lookup_conv1x1(c, w, bias)
    assert got.shape == (B, 96, H, W)
    assert_same_f32(got, ref.lookup_conv1x1(c, w, bias), f"case {case} r{r} conv1x1")
    assert (got != 0).any()
    for odt in (torch.float16, torch.bfloat16):
        assert_bit_equal(cb16.lookup_conv1x1(c, w, bias, out_dtype=odt), got, odt,
                         f"case {case} r{r} conv1x1 -> {odt}")


# ------------------------------------------------------------------- 5. range
@pytest.mark.parametrize("fdt,layout", [("f16", "nchw"), ("f16", "nhwc"), ("f32", "nchw")])
@pytest.mark.parametrize("case", ["a", "c"])
def test_pyr16_subnormal_cells_kept(dx, case, fdt, layout):
    """fmaps x 1e-3: every correlation (x 1e-6, max |cell| 2.2e-5 / 3.3e-5 in the
    float64 oracle) sits on float16's subnormal grid and must be stored as
    torch's .half() gives it, not flushed."""
    cb32 = _block(case, fdt, layout, "f32", 1e-3)
    a = cb32.corr_pyramid[0].abs()
    sub = (a >= 2.0 ** -25) & (a < F16_MIN_NORMAL)    # rounds to a non-zero float16 subnormal
    print(f"case {case}: {int(sub.sum())} of {sub.numel()} level-0 cells float16-subnormal")
    assert int(sub.sum().item()) > sub.numel() // 10
    h = cb32.corr_pyramid[0].half()
    assert int(((h != 0) & (h.abs() < F16_MIN_NORMAL)).sum().item()) > sub.numel() // 10
    assert_levels_are_half_of(_block(case, fdt, layout, "f16", 1e-3), cb32, f"case {case} x1e-3")


@pytest.mark.parametrize("fdt,layout", [("f16", "nchw"), ("f16", "nhwc"), ("f32", "nchw")])
def test_pyr16_overflow_to_inf(dx, fdt, layout):
    """Case c, fmaps x 60: the float32 pyramid is finite with cells beyond 65520,
    which the float16 pyramid stores as +-inf; a lookup that taps them returns
    inf / NaN exactly as the float32 lookup of the widened pyramid."""
    cb32 = _block("c", fdt, layout, "f32", OVERFLOW_SCALE)
    for lev in cb32.corr_pyramid:
        assert torch.isfinite(lev).all()
    n_over = [int((lev.abs() >= F16_OVERFLOW).sum().item()) for lev in cb32.corr_pyramid]
    print(f"scale {OVERFLOW_SCALE:g}: cells >= 65520 per level {n_over}")
    assert n_over[0] > 0 and n_over[3] > 0
    cb16 = _block("c", fdt, layout, "f16", OVERFLOW_SCALE)
    assert_levels_are_half_of(cb16, cb32, f"case c x{OVERFLOW_SCALE:g}")
    assert [int(torch.isinf(lev).sum().item()) for lev in cb16.corr_pyramid] == n_over
    c = _t(_coords("c"))
    got = cb16(c)
    assert torch.isinf(got).any()
    assert_same_f32(got, _widened_f32_block(cb16)(c), "lookup over +-inf cells")


# -------------------------------------------------------------- 6. loud paths
def test_pyr16_loud_paths(dx):
    f1h, f2h = _dev_fmaps("a", "f16")
    for a, b in ((f1h, f2h), (f1h.float(), f2h.float())):
        with pytest.raises(NotImplementedError, match="no gradient"):
            dx.CorrBlock(a.clone().requires_grad_(True), b, pyramid_dtype=torch.float16)
        with torch.no_grad():   # grad mode off: a plain inference block
            cb = dx.CorrBlock(a.clone().requires_grad_(True), b, pyramid_dtype=torch.float16)
        assert torch.equal(cb._buf.view(torch.int16),
                           _block("a", "f16", "nchw", "f16")._buf.view(torch.int16))
    g1 = _t(dg.fmap(1660, 1, 64, 32, 32, "fnet")).half()
    with pytest.raises(NotImplementedError, match="4 levels"):
        dx.CorrBlock(g1, g1, num_levels=5, pyramid_dtype=torch.float16)
    with pytest.raises(ValueError, match="bfloat16"):
        dx.CorrBlock(f1h.bfloat16(), f2h.bfloat16(), pyramid_dtype=torch.float16)
    with pytest.raises(ValueError, match="pyramid_dtype"):
        dx.CorrBlock(f1h, f2h, pyramid_dtype=torch.bfloat16)
    # defaults are what they were; torch.float32 names the default
    assert dx.CorrBlock(f1h, f2h)._buf.dtype == torch.float32
    assert dx.CorrBlock(f1h.float(), f2h.float())._buf.dtype == torch.float32
    assert dx.CorrBlock(f1h.bfloat16(), f2h.bfloat16())._buf.dtype == torch.bfloat16
    d = dx.CorrBlock(f1h, f2h, pyramid_dtype=torch.float32)
    assert d._buf.dtype == torch.float32
    assert torch.equal(d._buf, _block("a", "f16", "nchw", "f32")._buf)
    # the lookup backward and the pyramid backward take no float16 pyramid
    from dexiraft_amd import _native as nat
    cb = _block("a", "f16", "nchw", "f16")
    B, D, H, W = CASES["a"]
    c = _t(_coords("a"))
    go = torch.zeros((B, 4 * 81, H, W), device=DEV)
    assert nat.load().dxr_corr_lookup_backward(c.data_ptr(), go.data_ptr(), B, H, W, 4, 4,
                                               cb._buf.data_ptr(), nat.DXR_PYR_F16,
                                               nat.stream_of(c)) == nat.DXR_EINVAL


# ------------------------------------------------------ 7. accuracy statement
@pytest.mark.parametrize("scale", [1.0, 1e-3])
@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_pyr16_accuracy_against_float64(dx, case, scale):
    """Per cell, against the float64 oracle on the widened fmaps:
        |cell - ref| <= half a float16 ulp of ref + 1e-4 max|ref|
    with half an ulp = 2^-11 |ref| for normal results and 2^-25 (absolute) on the
    subnormal grid — one rounding to float16 on top of the float32 build's
    existing bar.  Derived from the number format, not measured."""
    cb16 = _block(case, "f16", "nchw", "f16", scale)
    ref = _ref64(case, scale)
    for lvl, lev in enumerate(cb16.corr_pyramid):
        got = lev[:, 0].cpu().numpy().astype(np.float64)
        r = ref[lvl]
        a = np.abs(r)
        half_ulp = np.where(a < F16_MIN_NORMAL, 2.0 ** -25, a * 2.0 ** -11)
        bound = half_ulp + RTOL * a.max()
        err = np.abs(got - r)
        print(f"case {case} x{scale:g} level {lvl}: max err {err.max():.3e}, max err/bound "
              f"{(err / bound).max():.3f}, max|ref| {a.max():.3e}")
        assert np.isfinite(got).all()
        assert (err <= bound).all()
