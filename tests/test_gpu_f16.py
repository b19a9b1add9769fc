"""GPU: float16 fmaps in CorrBlock (the single-product f16 record build, DXR_F16).

The reference everywhere is the float64 oracle on the WIDENED float16 values:
the reference model's arithmetic after its ``fmap.float()`` (core/raft.py:139-142).
Shapes are chosen from the kernel's structure (corr_build_dma_kernel, a stage =
32 channels, a unit = 2 x 128 queries x one 8x16 target tile):

  a  B=2 D=32  9x13   one K stage (nk = 1: no second prefetch); 117 queries = one
                      partial query block whose partner half is not live; ragged
                      8x16 target tiles, odd W; batch offset
  b  B=1 D=96  23x37  nk = 3: the ring fills exactly once; 851 queries: an odd
                      number of 128-query blocks plus tail quarter units
  c  B=1 D=256 16x24  nk = 8: the ring wraps; the production D
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest
import torch

import datagen as dg
import oracle
from conftest import tolerance_check

pytestmark = pytest.mark.gpu

RTOL = 1e-4
DEV = "cuda:0"
CASES = {"a": (2, 32, 9, 13), "b": (1, 96, 23, 37), "c": (1, 256, 16, 24)}
SEEDS = {"a": 1610, "b": 1620, "c": 1630}


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
    """fnet-like fmaps x scale, rounded to float16 (numpy float16 arrays)."""
    B, D, H, W = CASES[case]
    s = SEEDS[case]
    f1 = (dg.fmap(s, B, D, H, W, "fnet") * np.float32(scale)).astype(np.float16)
    f2 = (dg.fmap(s + 1, B, D, H, W, "fnet") * np.float32(scale)).astype(np.float16)
    return f1, f2


@lru_cache(maxsize=None)
def _ref(case: str, scale: float = 1.0):
    """float64 oracle pyramid of the widened float16 values (computed once)."""
    f1, f2 = _fmaps16(case, scale)
    return oracle.corr_pyramid(f1.astype(np.float32), f2.astype(np.float32), 4, np.float64)


def _levels(cb):
    return [lev[:, 0].cpu().numpy() for lev in cb.corr_pyramid]


# ------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_f16_parity(dx, case, layout):
    from dexiraft_amd import _native as nat
    B, D, H, W = CASES[case]
    f1n, f2n = _fmaps16(case)
    f1, f2 = _t(f1n), _t(f2n)
    assert f1.dtype == torch.float16
    nchw = dx.CorrBlock(f1, f2)
    cb = nchw if layout == "nchw" else dx.CorrBlock(_cl(f1), _cl(f2))
    assert cb._buf.dtype == torch.float32
    ref = _ref(case)
    for lvl, got in enumerate(_levels(cb)):
        e = tolerance_check(got, ref[lvl], RTOL)
        print(f"case {case} {layout} level {lvl}: err/max {e:.3e}")
    c = dg.coords(SEEDS[case] + 2, B, H, W, "uniform", 6.0)   # windows partly off the map
    out = cb(_t(c))
    assert out.dtype == torch.float32 and out.is_contiguous()
    e = tolerance_check(out.cpu().numpy(), oracle.corr_lookup(ref, c, 4), RTOL)
    print(f"case {case} {layout} lookup: err/max {e:.3e}")
    # NCHW and channels-last fmaps of the same values: the same bits
    assert torch.equal(cb._buf, nchw._buf)
    # the library itself took DXR_F16 (no quiet widening in the Python layer)
    lib = nat.load()
    g1, g2 = (f1, f2) if layout == "nchw" else (_cl(f1), _cl(f2))
    code = nat.DXR_NCHW if layout == "nchw" else nat.DXR_NHWC
    nbytes = lib.dxr_build_workspace_bytes(nat.DXR_F16, B, D, H, W) if layout == "nchw" else 0
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)
    buf = torch.full_like(nchw._buf, float("nan"))
    st = lib.dxr_corr_pyramid_build_ws(g1.data_ptr(), g2.data_ptr(), nat.DXR_F16, code, B, D, H, W,
                                       4, float(np.sqrt(np.float32(D))), buf.data_ptr(),
                                       nat.DXR_F32, nat.DXR_BUILD_AUTO,
                                       ws.data_ptr() if nbytes else None, nbytes,
                                       nat.stream_of(buf))
    assert st == nat.DXR_OK
    torch.cuda.synchronize()
    assert torch.equal(buf, nchw._buf)


# --------------------------------------------------------------- 2. f32 class
def _exact_f32_levels(f1: torch.Tensor, f2: torch.Tensor):
    """The exact-f32 MFMA build (DXR_BUILD_EXACT_F32; not under test) of f32 fmaps."""
    from dexiraft_amd import _native as nat
    lib = nat.load()
    B, D, H, W = (int(v) for v in f1.shape)
    buf = torch.empty(lib.dxr_pyramid_numel(B, H, W, 4), device=DEV)
    st = lib.dxr_corr_pyramid_build(f1.data_ptr(), f2.data_ptr(), nat.DXR_F32, nat.DXR_NCHW, B, D,
                                    H, W, 4, float(np.sqrt(np.float32(D))), buf.data_ptr(),
                                    nat.DXR_F32, nat.DXR_BUILD_EXACT_F32, nat.stream_of(f1))
    assert st == 0
    out, h, w = [], H, W
    for lvl in range(4):
        if lvl:
            h, w = h // 2, w // 2
        t = torch.empty((B * H * W, h, w), device=DEV)
        assert lib.dxr_pyramid_unpack(buf.data_ptr(), nat.DXR_F32, B, H, W, 4, lvl, t.data_ptr(),
                                      nat.stream_of(t)) == 0
        out.append(t.cpu().numpy())
    return out


@pytest.mark.parametrize("scale", [1.0, 1e-3, 60.0])
@pytest.mark.parametrize("case", ["b", "c"])
def test_f16_build_is_f32_class(dx, case, scale):
    """Per level, the f16 build's max error against float64 is within 2x the
    exact-f32 MFMA build's on the widened inputs, + 1e-7 max|ref| (the bar of
    test_prescaled_split_build_accuracy_is_scale_free: a different summation
    order and nothing else).  1e-3 puts the small values on float16's subnormal
    grid (the MFMA must not flush them); 60 brings the largest near 3e2."""
    f1n, f2n = _fmaps16(case, scale)
    ref = _ref(case, scale)
    f1, f2 = _t(f1n), _t(f2n)
    base = _exact_f32_levels(f1.float(), f2.float())
    got = _levels(dx.CorrBlock(f1, f2))
    for lvl in range(4):
        e16 = np.abs(got[lvl] - ref[lvl]).max()
        e32 = np.abs(base[lvl] - ref[lvl]).max()
        m = np.abs(ref[lvl]).max()
        print(f"case {case} scale {scale:g} level {lvl}: max|err| f16 build {e16:.3e}, exact f32 "
              f"{e32:.3e}, max|ref| {m:.3e}")
        assert e16 <= 2 * e32 + 1e-7 * m


# ------------------------------------------- 3. the f32 path's bits at unit scale
def test_f16_build_equals_f32_path_at_unit_scale(dx):
    """Case c: the f16 record build and the f32 pair build on the widened values
    give the same pyramid bit for bit — the prescale only scales these pixels up
    (exact), lo = 0 adds exact zeros, each accumulator sees the same 16-channel
    blocks in the same order, and the scales are powers of two."""
    f1n, f2n = _fmaps16("c")
    f1, f2 = _t(f1n), _t(f2n)
    a = dx.CorrBlock(f1, f2)._buf
    b = dx.CorrBlock(f1.float(), f2.float())._buf
    d = (a - b).abs().max().item()
    print(f"max |f16 build - f32 path| = {d:.3e} (max|ref| {b.abs().max().item():.3e})")
    assert torch.equal(a, b)


# ------------------------------------------------------ 4. non-finite operands
def test_f16_nonfinite_operands(dx):
    B, D, H, W = CASES["b"]
    f1n, f2n = (x.copy() for x in _fmaps16("b"))
    f1n[0, 5, 3, 7] = np.inf
    f2n[0, 40, 11, 20] = np.nan
    f1n[0, 77, 19, 30] = np.float16(65504.0)
    f1, f2 = _t(f1n), _t(f2n)
    got = _levels(dx.CorrBlock(f1, f2))
    wide = _levels(dx.CorrBlock(f1.float(), f2.float()))
    with np.errstate(invalid="ignore", over="ignore"):
        ref = oracle.corr_pyramid(f1n.astype(np.float32), f2n.astype(np.float32), 4, np.float64)
    for lvl in range(4):
        assert np.array_equal(np.isnan(got[lvl]), np.isnan(wide[lvl])), lvl
        assert np.array_equal(np.isposinf(got[lvl]), np.isposinf(wide[lvl])), lvl
        assert np.array_equal(np.isneginf(got[lvl]), np.isneginf(wide[lvl])), lvl
        fin = np.isfinite(wide[lvl])
        assert 0 < (~fin).sum() < fin.size
        assert np.isfinite(ref[lvl][fin]).all(), lvl
        e = tolerance_check(got[lvl][fin], ref[lvl][fin], RTOL)
        print(f"level {lvl}: {(~fin).sum()} non-finite cells, finite err/max {e:.3e}")


# ------------------------------------------------- 5. fallbacks and refusals
def test_f16_d48_takes_the_widened_f32_path(dx):
    f1 = _t(dg.fmap(1650, 2, 48, 9, 13, "fnet")).half()
    f2 = _t(dg.fmap(1651, 2, 48, 9, 13, "fnet")).half()
    a, b = dx.CorrBlock(f1, f2), dx.CorrBlock(f1.float(), f2.float())
    assert a._buf.dtype == torch.float32
    assert torch.equal(a._buf, b._buf)
    assert torch.equal(dx.CorrBlock(_cl(f1), _cl(f2))._buf, b._buf)


def test_f16_five_levels(dx):
    B, D, H, W = 1, 64, 32, 32
    f1n = dg.fmap(1660, B, D, H, W, "fnet").astype(np.float16)
    f2n = dg.fmap(1661, B, D, H, W, "fnet").astype(np.float16)
    ref = oracle.corr_pyramid(f1n.astype(np.float32), f2n.astype(np.float32), 5, np.float64)
    for f1, f2 in ((_t(f1n), _t(f2n)), (_cl(_t(f1n)), _cl(_t(f2n)))):
        cb = dx.CorrBlock(f1, f2, num_levels=5)
        got = _levels(cb)
        assert len(got) == 5 and got[4].shape[1:] == (2, 2)
        for lvl in range(5):
            tolerance_check(got[lvl], ref[lvl], RTOL)
        c = dg.coords(1662, B, H, W, "normal", 4.0)
        tolerance_check(cb(_t(c)).cpu().numpy(), oracle.corr_lookup(ref, c, 4), RTOL)


def test_f16_requires_grad_raises(dx):
    f1n, f2n = _fmaps16("a")
    f1, f2 = _t(f1n).requires_grad_(True), _t(f2n)
    with pytest.raises(NotImplementedError):
        dx.CorrBlock(f1, f2)
    with torch.no_grad():
        cb = dx.CorrBlock(f1, f2)
    assert torch.equal(cb._buf, dx.CorrBlock(f1.detach(), f2)._buf)


def test_f16_alternate_block_widens_exactly(dx):
    B, D, H, W = 1, 64, 24, 40
    f1 = _t(dg.fmap(1670, B, D, H, W, "fnet")).half()
    f2 = _t(dg.fmap(1671, B, D, H, W, "fnet")).half()
    c = _t(dg.coords(1672, B, H, W, "normal", 4.0))
    a = dx.AlternateCorrBlock(f1, f2)(c)
    b = dx.AlternateCorrBlock(f1.float(), f2.float())(c)
    assert a.dtype == torch.float32
    assert torch.equal(a, b)
    ref = oracle.corr_lookup(oracle.corr_pyramid(f1.float().cpu().numpy(), f2.float().cpu().numpy(),
                                                 4, np.float64), c.cpu().numpy(), 4)
    tolerance_check(a.cpu().numpy(), ref, RTOL)


def test_f16_lookup_conv1x1(dx):
    B, D, H, W = CASES["c"]
    f1n, f2n = _fmaps16("c")
    f1, f2 = _t(f1n), _t(f2n)
    c = _t(dg.coords(1680, B, H, W, "normal", 4.0))
    w, bias = dg.conv1x1_weights(3, 96, 4 * 81)
    a = dx.CorrBlock(f1, f2).lookup_conv1x1(c, _t(w), _t(bias))
    b = dx.CorrBlock(f1.float(), f2.float()).lookup_conv1x1(c, _t(w), _t(bias))
    assert a.shape == (B, 96, H, W)
    tolerance_check(a.cpu().numpy(), b.cpu().numpy(), RTOL)


# ------------------------------------------------------------- 6. end to end
def test_f16_e2e_flow_matches_f32_block_on_the_same_values(dx):
    """The 12-iteration refinement loop (tests/e2e_flow.py) at its own shape: the
    float16 block against the f32 CorrBlock fed the same float16-rounded fmaps,
    widened.  Final-flow EPE < 1e-3 px (north star C1)."""
    import e2e_flow as ef
    from test_e2e_flow import EPE_F32, _run

    def widened(f1, f2):
        assert f1.dtype == torch.float16
        return dx.CorrBlock(f1.float(), f2.float())

    def direct(f1, f2):
        assert f1.dtype == torch.float16
        return dx.CorrBlock(f1, f2)

    flows_a, up_a, e_a = _run(direct, "cuda", torch.float16)
    flows_b, up_b, e_b = _run(widened, "cuda", torch.float16)
    per_iter = [ef.epe(x, y) for x, y in zip(flows_a, flows_b)]
    print(f"final EPE {per_iter[-1]:.3e} px, max over iters {max(per_iter):.3e}, "
          f"edge flow {ef.epe(e_a, e_b):.3e}")
    assert np.isfinite(per_iter[-1])
    assert per_iter[-1] < EPE_F32
    assert ef.epe(e_a, e_b) < EPE_F32
