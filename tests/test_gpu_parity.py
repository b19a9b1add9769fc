"""GPU parity tests: HIP kernels (through the C-ABI) vs the reference's golden
vectors and the oracle.  Tolerances (north star, BASELINE.json):
  * fp32 pyramid: |ours - ref| <= 1e-4 * max|ref| per level;
  * lookup on our own pyramid: same 1e-4-of-max bound;
  * lookup on the reference's pyramid: bit-exact (same arithmetic as ATen's CPU
    grid sampler, incl. its fused-multiply-add chain);
  * integer/index properties (symmetry, batching, determinism, pooling of an
    exactly representable volume): bit-exact.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import datagen as dg
import oracle
from conftest import large_cases, load_large, load_tiny, tiny_cases, tolerance_check

pytestmark = pytest.mark.gpu

RTOL = 1e-4
DEV = "cuda:0"


@pytest.fixture(scope="module")
def dx():
    import dexiraft_amd
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    dexiraft_amd.load_native()
    return dexiraft_amd


def _t(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# --------------------------------------------------------------------------- tiny cases
@pytest.mark.parametrize("name", tiny_cases())
def test_pyramid_matches_reference(dx, name):
    d = load_tiny(name)
    cb = dx.CorrBlock(_t(d["fmap1"]), _t(d["fmap2"]), num_levels=d["num_levels"], radius=d["radius"])
    rows = torch.from_numpy(d["pyr_rows"]).to(DEV)
    assert len(cb.corr_pyramid) == d["num_levels"]
    for lvl in range(d["num_levels"]):
        ref = d[f"pyr{lvl}"]
        got = cb.corr_pyramid[lvl][rows, 0].cpu().numpy()
        tolerance_check(got, ref, RTOL)


@pytest.mark.parametrize("name", tiny_cases())
def test_lookup_matches_reference(dx, name):
    d = load_tiny(name)
    cb = dx.CorrBlock(_t(d["fmap1"]), _t(d["fmap2"]), num_levels=d["num_levels"], radius=d["radius"])
    for k in range(d["n_coords"]):
        out = cb(_t(d[f"coords{k}"]))
        assert out.is_contiguous() and out.dtype == torch.float32
        tolerance_check(out.cpu().numpy(), d[f"out{k}"], RTOL)


@pytest.mark.parametrize("name", [n for n in tiny_cases()
                                  if len(load_tiny(n)["pyr_rows"]) == load_tiny(n)["B"] *
                                  load_tiny(n)["H"] * load_tiny(n)["W"]])
def test_lookup_bitexact_on_reference_pyramid(dx, name):
    """dxr_corr_lookup on the reference's own pyramid reproduces its bits.  The
    reference levels are packed into a NaN-prefilled paged buffer (packing writes
    only real cells), so any read of page padding would surface as NaN."""
    d = load_tiny(name)
    from dexiraft_amd import _native as nat
    lib = nat.load()
    B, H, W, L, r = d["B"], d["H"], d["W"], d["num_levels"], d["radius"]
    buf = torch.full((lib.dxr_pyramid_numel(B, H, W, L),), float("nan"), device=DEV)
    for lvl in range(L):
        lev = _t(d[f"pyr{lvl}"])
        st = lib.dxr_pyramid_pack(lev.data_ptr(), B, H, W, L, lvl, buf.data_ptr(), nat.DXR_F32,
                                  nat.stream_of(lev))
        assert st == 0
        back = torch.empty_like(lev)
        st = lib.dxr_pyramid_unpack(buf.data_ptr(), nat.DXR_F32, B, H, W, L, lvl,
                                    back.data_ptr(), nat.stream_of(lev))
        assert st == 0 and torch.equal(back, lev)          # pack/unpack round trip
    rd = 2 * r + 1
    for k in range(d["n_coords"]):
        c = _t(d[f"coords{k}"])
        out = torch.empty((B, L * rd * rd, H, W), device=DEV)
        st = lib.dxr_corr_lookup(buf.data_ptr(), nat.DXR_F32, B, H, W, L, r, c.data_ptr(),
                                 out.data_ptr(), nat.stream_of(c))
        assert st == 0
        got, ref = out.cpu().numpy(), d[f"out{k}"]
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        fin = ~np.isnan(ref)
        assert np.array_equal(got[fin], ref[fin]), \
            f"max diff {np.abs(got[fin] - ref[fin]).max():.3e}"


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_lookup_grid_shapes_agree_on_padded_pyramid(dx, dtype):
    """Round 6: the query-minor lookup runs one-round grids (256 x 16, plain
    loads) and multi-round grids (512 x 32, range-checked buffer loads).  A B=6
    batch at Chairs size (level widths 62, 31, 15, 7: partial 4-cell vectors on
    every level; N % 32 = 4: a partial query block) runs the multi-round form;
    each pair alone runs the one-round form.  On a NaN-prefilled paged buffer
    (any read of page padding would surface as NaN) both give the same bits,
    with normal, integer, uniform (many taps off the map), far and non-finite
    coordinates; pair 0 also against the oracle's lookup (bit-exact, f32)."""
    from dexiraft_amd import _native as nat
    lib = nat.load()
    B, D, H, W, L, r = 6, 256, 46, 62, 4, 4
    f1, f2 = _pair(B=B, D=D, H=H, W=W, seed=411, dist="fnet")
    cb = dx.CorrBlock(f1, f2)
    levels = [cb.corr_pyramid[lvl] for lvl in range(L)]        # reference layout, f32
    pdt = nat.DXR_F32 if dtype == "f32" else nat.DXR_BF16
    n = lib.dxr_pyramid_numel(B, H, W, L)
    buf = torch.full((n,), float("nan"), device=DEV,
                     dtype=torch.float32 if dtype == "f32" else torch.bfloat16)
    for lvl in range(L):
        lev = levels[lvl].contiguous()
        assert lib.dxr_pyramid_pack(lev.data_ptr(), B, H, W, L, lvl, buf.data_ptr(), pdt,
                                    nat.stream_of(lev)) == 0
    cs = [dg.coords(500 + i, B, H, W, m, s) for i, (m, s) in
          enumerate([("normal", 4.0), ("integer", 4.0), ("uniform", 30.0), ("far", 4.0)])]
    bad = dg.coords(510, B, H, W, "normal", 4.0)
    bad[0, 0, 3, 5], bad[1, 1, 7, 7], bad[2, 0, 0, 0] = np.nan, np.inf, -np.inf
    cs.append(bad)
    K = L * (2 * r + 1) ** 2
    N = H * W
    singles = []   # each pair packed alone (B=1 buffers: the one-round grid)
    for b in range(B):
        b1 = torch.full((lib.dxr_pyramid_numel(1, H, W, L),), float("nan"), device=DEV,
                        dtype=buf.dtype)
        for lvl in range(L):
            lev = levels[lvl][b * N:(b + 1) * N].contiguous()
            assert lib.dxr_pyramid_pack(lev.data_ptr(), 1, H, W, L, lvl, b1.data_ptr(), pdt,
                                        nat.stream_of(lev)) == 0
        singles.append(b1)
    for c in cs:
        ct = _t(c)
        many = torch.empty((B, K, H, W), device=DEV)
        assert lib.dxr_corr_lookup(buf.data_ptr(), pdt, B, H, W, L, r, ct.data_ptr(),
                                   many.data_ptr(), nat.stream_of(ct)) == 0
        for b in range(B):
            cb1 = ct[b:b + 1].contiguous()
            one = torch.empty((1, K, H, W), device=DEV)
            assert lib.dxr_corr_lookup(singles[b].data_ptr(), pdt, 1, H, W, L, r,
                                       cb1.data_ptr(), one.data_ptr(), nat.stream_of(ct)) == 0
            assert torch.equal(torch.nan_to_num(one[0], nan=7.0), torch.nan_to_num(many[b], nan=7.0)), b
        if dtype == "f32":
            pyr0 = [levels[lvl][: H * W, 0].cpu().numpy() for lvl in range(L)]
            ref = oracle.corr_lookup(pyr0, c[:1], r)
            got = many[:1].cpu().numpy()
            assert np.array_equal(np.isnan(got), np.isnan(ref))
            assert np.array_equal(got[~np.isnan(ref)], ref[~np.isnan(ref)])


@pytest.mark.parametrize("name", ["fnet", "ragged", "levels2_r1"])
def test_corr_static_method(dx, name):
    d = load_tiny(name)
    vol = dx.CorrBlock.corr(_t(d["fmap1"]), _t(d["fmap2"]))
    B, H, W = d["B"], d["H"], d["W"]
    assert tuple(vol.shape) == (B, H, W, 1, H, W)
    got = vol.reshape(B * H * W, H, W)[torch.from_numpy(d["pyr_rows"]).to(DEV)].cpu().numpy()
    tolerance_check(got, d["pyr0"], RTOL)


# --------------------------------------------------------------------------- benchmark shapes
@pytest.mark.parametrize("name", large_cases())
def test_large_shapes_against_reference_checksums(dx, name):
    d = load_large(name)
    B, D, H, W, r = d["B"], d["D"], d["H"], d["W"], d["radius"]
    f1 = dg.fmap(d["fmap_seeds"][0], B, D, H, W, d["dist"])
    f2 = dg.fmap(d["fmap_seeds"][1], B, D, H, W, d["dist"])
    # generator drift would invalidate the comparison: pin the inputs first
    np.testing.assert_allclose([f1.astype(np.float64).sum(), f2.astype(np.float64).sum()],
                               d["fmap_checksum"], rtol=0, atol=1e-6)
    cb = dx.CorrBlock(_t(f1), _t(f2), radius=r)
    for lvl in range(4):
        a = cb.corr_pyramid[lvl].reshape(-1)
        maxabs = float(d[f"pyr{lvl}_maxabs"])
        got = a[torch.from_numpy(d[f"pyr{lvl}_idx"]).to(DEV)].cpu().numpy()
        assert np.abs(got - d[f"pyr{lvl}_val"]).max() <= RTOL * maxabs
        s = a.double().sum().item()
        s2 = (a.double() ** 2).sum().item()
        ref_s, ref_s2 = d[f"pyr{lvl}_sum"]
        # Bias guard: a systematic error shows up linearly in a 10^7-cell sum,
        # random rounding only as sqrt(n).  MFMAs align and truncate their addends
        # inside the f32 accumulator: r01's 3-way bf16 split showed a mean error of
        # -2.7e-9 max|ref| at Sintel (a round-1 GPU diagnostic, retired since), i.e.
        # 3.7e4x under the 1e-4 per-cell tolerance; bound it at 1e-8 max|ref| per cell.
        # (The bias is per cell of level 0 and pooling keeps it: scale by level 0's max.)
        assert abs(s - ref_s) <= 1e-6 * abs(ref_s) + 1e-8 * a.numel() * float(d["pyr0_maxabs"])
        assert abs(s2 - ref_s2) <= 1e-5 * ref_s2
        assert abs(a.abs().max().item() - maxabs) <= RTOL * maxabs
    for k, (mode, scale, seed) in enumerate(d["coords"]):
        c = dg.coords(int(seed), B, H, W, mode, float(scale))
        assert abs(c.astype(np.float64).sum() - float(d[f"coords{k}_checksum"])) < 1e-3
        out = cb(_t(c))
        maxabs = float(d[f"out{k}_maxabs"])
        got = out.reshape(-1)[torch.from_numpy(d[f"out{k}_idx"]).to(DEV)].cpu().numpy()
        assert np.abs(got - d[f"out{k}_val"]).max() <= RTOL * maxabs
        chsum = out.double().sum(dim=(0, 2, 3)).cpu().numpy()
        np.testing.assert_allclose(chsum, d[f"out{k}_chsum"], rtol=0,
                                   atol=1e-6 * B * H * W * maxabs)


# --------------------------------------------------------------------------- properties
def _pair(B=1, D=256, H=55, W=128, seed=0, dist="normal"):
    return (_t(dg.fmap(seed, B, D, H, W, dist)), _t(dg.fmap(seed + 1, B, D, H, W, dist)))


def test_symmetry_bitexact(dx):
    """corr(f1, f2)[i, j] == corr(f2, f1)[j, i]: same k-ordered f32 chain."""
    f1, f2 = _pair(H=23, W=40, seed=3)
    a = dx.CorrBlock.corr(f1, f2).reshape(920, 920)
    b = dx.CorrBlock.corr(f2, f1).reshape(920, 920)
    assert torch.equal(a, b.t())


def test_batch_independence_and_determinism(dx):
    f1, f2 = _pair(B=3, H=30, W=44, seed=5, dist="fnet")
    cbb = dx.CorrBlock(f1, f2)
    cbb2 = dx.CorrBlock(f1, f2)
    c = _t(dg.coords(9, 3, 30, 44, "normal", 4.0))
    ob = cbb(c)
    assert torch.equal(ob, cbb2(c))
    for lvl in range(4):
        assert torch.equal(cbb.corr_pyramid[lvl], cbb2.corr_pyramid[lvl])
    n = 30 * 44
    for b in range(3):
        cb1 = dx.CorrBlock(f1[b:b + 1], f2[b:b + 1])
        for lvl in range(4):
            assert torch.equal(cb1.corr_pyramid[lvl], cbb.corr_pyramid[lvl][b * n:(b + 1) * n])
        assert torch.equal(cb1(c[b:b + 1]), ob[b:b + 1])


@pytest.mark.parametrize("dtype,B", [(torch.float32, 2), (torch.bfloat16, 4)])
def test_pyramid_store_policy_bit_identical(dx, dtype, B):
    """The DMA builds pick their pyramid stores per launch (csrc/corr_build.hip
    dma_stream_out): write-through up to 512 MB of pyramid, non-temporal above.
    At Sintel size a one-pair pyramid is below the threshold (f32 269 MB, bf16
    135 MB) and this batch above it (538 MB): every slot's pages and lookups must
    be the one-pair build's bit for bit."""
    H, W = 55, 128
    f1, f2 = _pair(B=B, H=H, W=W, seed=21, dist="fnet")
    f1, f2 = f1.to(dtype), f2.to(dtype)
    c = _t(dg.coords(22, B, H, W, "normal", 4.0))
    cbb = dx.CorrBlock(f1, f2)
    ob = cbb(c)
    pyr = cbb.corr_pyramid
    n = H * W
    for b in range(B):
        cb1 = dx.CorrBlock(f1[b:b + 1], f2[b:b + 1])
        for lvl in range(4):
            assert torch.equal(cb1.corr_pyramid[lvl], pyr[lvl][b * n:(b + 1) * n]), (b, lvl)
        assert torch.equal(cb1(c[b:b + 1]), ob[b:b + 1]), b
        del cb1


def test_linearity(dx):
    """Scaling fmap1 by 2 scales the pyramid by 2 (the reference's f32 matmul does
    so bit for bit).  Bit for bit on the default (pre-split) build, whose
    per-pixel power-of-two scaling absorbs the factor, and on the exact-f32
    build; the r02 workspace-less split build (unscaled f16 pairs) only to within
    2^-20 of max|.|: its residuals below 2^-14 round on f16's fixed subnormal
    grid, which doubling does not commute with."""
    f1, f2 = _pair(H=21, W=36, seed=11)
    a = dx.CorrBlock(f1, f2)
    b = dx.CorrBlock(2.0 * f1, f2)
    c = dx.CorrBlock(f1, 0.25 * f2)
    for lvl in range(4):
        assert torch.equal(b.corr_pyramid[lvl], 2.0 * a.corr_pyramid[lvl]), lvl
        assert torch.equal(c.corr_pyramid[lvl], 0.25 * a.corr_pyramid[lvl]), lvl
    ea, eb = _build_exact_f32(f1, f2), _build_exact_f32(2.0 * f1, f2)
    for lvl in range(4):
        assert torch.equal(eb[lvl], 2.0 * ea[lvl])
    sa, sb = _build_no_workspace(f1, f2), _build_no_workspace(2.0 * f1, f2)
    for lvl in range(4):
        d = (sb[lvl] - 2.0 * sa[lvl]).abs().max().item()
        assert d <= 2.0 ** -20 * sa[lvl].abs().max().item(), (lvl, d)


def test_fused_pooling_matches_torch_avg_pool(dx):
    f1, f2 = _pair(H=55, W=128, seed=21)
    cb = dx.CorrBlock(f1, f2)
    for lvl in range(1, 4):
        ref = torch.nn.functional.avg_pool2d(cb.corr_pyramid[lvl - 1], 2, stride=2)
        assert ref.shape == cb.corr_pyramid[lvl].shape
        err = (ref - cb.corr_pyramid[lvl]).abs().max().item()
        assert err <= 1e-6 * ref.abs().max().item()


def test_integer_coords_sample_cells(dx):
    """At integer coordinates the centre tap is the pyramid cell itself, up to the
    few-ulp shift of the reference's normalise/unnormalise round trip."""
    H, W = 40, 52
    f1, f2 = _pair(H=H, W=W, seed=31)
    cb = dx.CorrBlock(f1, f2)
    c = _t(dg.coords(33, 1, H, W, "integer", 5.0))
    out = cb(c)
    cx = c[0, 0].long().reshape(-1)
    cy = c[0, 1].long().reshape(-1)
    ok = (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
    q = torch.arange(H * W, device=DEV)
    lvl0 = cb.corr_pyramid[0][:, 0]
    centre = out[0, 4 * 9 + 4].reshape(-1)  # ix = iy = r at level 0
    ref = lvl0[q[ok], cy[ok], cx[ok]]
    assert (centre[ok] - ref).abs().max().item() <= 1e-5 * lvl0.abs().max().item()
    assert ok.float().mean().item() > 0.5
    assert (centre[~ok].abs() <= 1e-5 * lvl0.abs().max().item()).all()


def test_far_coords_give_zero_and_nan_coords_give_nan(dx):
    f1, f2 = _pair(H=20, W=24, seed=41)
    cb = dx.CorrBlock(f1, f2)
    c = _t(dg.coords(43, 1, 20, 24, "far"))
    assert torch.all(cb(c) == 0)
    c2 = c.clone()
    c2[0, 0, 3, 5] = float("nan")
    o = cb(c2)
    assert torch.all(torch.isnan(o[0, :, 3, 5]))
    assert not torch.isnan(o[0, :, 3, 6]).any()
    c3 = c.clone()
    c3[0, 1, 0, 0] = float("inf")
    assert torch.all(torch.isnan(cb(c3)[0, :, 0, 0]))


def test_full_size_against_oracle_float64(dx):
    """Sintel shape, fnet-like data: whole pyramid + one lookup vs the float64 oracle."""
    H, W = 55, 128
    f1 = dg.fmap(51, 1, 256, H, W, "fnet")
    f2 = dg.fmap(52, 1, 256, H, W, "fnet")
    c = dg.coords(53, 1, H, W, "normal", 4.0)
    pyr = oracle.corr_pyramid(f1, f2, 4, np.float64)
    cb = dx.CorrBlock(_t(f1), _t(f2))
    for lvl in range(4):
        tolerance_check(cb.corr_pyramid[lvl][:, 0].cpu().numpy(), pyr[lvl], RTOL)
    ref = oracle.corr_lookup(pyr, c, 4)
    tolerance_check(cb(_t(c)).cpu().numpy(), ref, RTOL)


# --------------------------------------------------------------------------- alternate path
def test_alternate_block_matches_reference_corrblock(dx):
    d = load_tiny("batch2_alt")
    ab = dx.AlternateCorrBlock(_t(d["fmap1"]), _t(d["fmap2"]), radius=d["radius"])
    assert len(ab.pyramid) == 5
    for k in range(d["n_coords"]):
        tolerance_check(ab(_t(d[f"coords{k}"])).cpu().numpy(), d[f"out{k}"], RTOL)


@pytest.mark.parametrize("shape", [(1, 64, 24, 32, 4), (2, 37, 17, 19, 3)])
def test_alternate_block_matches_oracle(dx, shape):
    B, D, H, W, r = shape
    f1 = dg.fmap(61, B, D, H, W)
    f2 = dg.fmap(62, B, D, H, W)
    c = dg.coords(63, B, H, W, "uniform", 9.0)
    ref = oracle.alt_corr_block(f1, f2, c, 4, r, np.float64)
    got = dx.AlternateCorrBlock(_t(f1), _t(f2), radius=r)(_t(c)).cpu().numpy()
    tolerance_check(got, ref, RTOL)


def test_alternate_block_overflow_fallback(dx):
    """The on-the-fly kernel's f16 pair split covers |x| < 65520; a chunk whose sums
    are not finite is recomputed on the 3-way bf16 split.  Operands of 1e5 (a whole
    query pixel) and 3e6 (one target channel) stay f32-class per query, and a NaN
    query yields NaN outputs for that query only, as the reference's f32 kernel."""
    B, D, H, W = 1, 64, 24, 32
    f1 = dg.fmap(65, B, D, H, W)
    f2 = dg.fmap(66, B, D, H, W)
    f1[0, :, 5, 7] *= 1.0e5
    f2[0, 3, 10, 12] = 3.0e6
    c = dg.coords(67, B, H, W, "normal", 3.0)
    ref = oracle.alt_corr_block(f1, f2, c, 4, 4, np.float64)
    got = dx.AlternateCorrBlock(_t(f1), _t(f2), radius=4)(_t(c)).cpu().numpy()
    assert np.isfinite(got).all()
    scale = np.abs(ref).max(axis=1, keepdims=True) + 1e-30      # per query pixel
    assert (np.abs(got - ref) <= 1e-4 * scale).all()
    assert np.abs(got[0, :, 5, 7]).max() > 1.0e4                 # the scaled query itself
    f1[0, 0, 2, 3] = np.nan
    ref = oracle.alt_corr_block(f1, f2, c, 4, 4, np.float64)
    got = dx.AlternateCorrBlock(_t(f1), _t(f2), radius=4)(_t(c)).cpu().numpy()
    nan_ref = np.isnan(ref)
    assert np.isnan(got[0, :, 2, 3]).any()
    fin = ~nan_ref
    assert np.isfinite(got[fin]).all()
    scale = np.broadcast_to(np.nanmax(np.abs(ref), axis=1, keepdims=True), ref.shape)
    assert (np.abs(got[fin] - ref[fin]) <= 1e-4 * scale[fin] + 1e-30).all()


def _alt_flow(B, H, W, flow, seed):
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32),
                         indexing="ij")
    grid = np.stack([xs, ys])[None].repeat(B, 0)
    rng = np.random.default_rng(seed)
    c = (grid + rng.normal(0, 4, size=grid.shape)).astype(np.float32)
    if flow == "far":
        c[:, 0, 3, 5] = np.nan
        c[:, 1, 7, 9] = np.inf
        c[:, :, 10, 2:30:3] = -40.0
        c[:, 0, 12, :20] = 3.0e9
    return _t(np.ascontiguousarray(c))


@pytest.mark.parametrize("flow", ["iid", "far"])
@pytest.mark.parametrize("shape", [(1, 256, 55, 128, 4), (2, 64, 30, 44, 3), (1, 256, 136, 240, 4)])
def test_alt_coarse_volumes_match_on_the_fly(dx, flow, shape, monkeypatch):
    """Round 6: AlternateCorrBlock can compute its coarse levels once per block
    as whole volumes of the same f16-pair MFMA dot products
    (dxr_alt_coarse_volumes: the tiled GEMM alt_volume_gemm_kernel) and read
    their windows with the reference's alt arithmetic (dxr_alt_volume_lookup);
    forced here from level 1 on (8x16 >> 1 .. 1x2 tiles), the outputs are the
    all-on-the-fly block's bit for bit, NaN / inf / off-image coordinates
    included.  The default policy (large maps, levels of <= 2,048 cells) picks
    levels 2-3 at 1080p and none at Sintel."""
    B, D, H, W, r = shape
    f1 = _t(dg.fmap(81, B, D, H, W, "fnet"))
    f2 = _t(dg.fmap(82, B, D, H, W, "fnet"))
    c = _alt_flow(B, H, W, flow, 83)
    # the default policy: volumes only on large maps, for levels of <= 2,048 cells
    assert dx.AlternateCorrBlock(f1, f2, radius=r).coarse_first_level == (2 if H > 100 else None)
    monkeypatch.setattr(dx.AlternateCorrBlock, "COARSE_MIN_QUERIES", 0)
    monkeypatch.setattr(dx.AlternateCorrBlock, "COARSE_LEVEL_MAX_CELLS", 1 << 20)
    monkeypatch.setattr(dx.AlternateCorrBlock, "COARSE_VOLUME_MAX_BYTES", 1 << 32)
    hyb = dx.AlternateCorrBlock(f1, f2, radius=r)
    assert hyb.coarse_first_level == 1
    monkeypatch.setattr(dx.AlternateCorrBlock, "COARSE_LEVEL_MAX_CELLS", 0)
    fly = dx.AlternateCorrBlock(f1, f2, radius=r)
    assert fly.coarse_first_level is None
    a, b = hyb(c), fly(c)
    assert torch.equal(torch.isnan(a), torch.isnan(b))
    assert torch.equal(torch.nan_to_num(a, nan=3.0), torch.nan_to_num(b, nan=3.0))
    assert torch.isfinite(a[0, :, 20, 40]).all()


@pytest.mark.parametrize("case", ["finite", "nonfinite"])
def test_alt_volume_gemm_against_float64(dx, case):
    """Round 6: the coarse-level volumes' tiled GEMM (alt_volume_gemm_kernel,
    levels 0-3: 8x16 .. 1x2 tiles, ragged level edges, a partial last query
    page, two pairs, D = 96; its register-split and LDS-DMA forms bit for bit
    alike) against float64 dot products of fmap1 with the
    pooled fmap2 levels: within 1e-5 of sum |a||b| per cell.  "nonfinite": a
    channel of 1e5 (beyond the f16 pair's range: its tiles re-run on the bf16
    split, and stay accurate), a NaN fmap2 pixel and an inf fmap1 pixel — the
    volume is non-finite exactly where float64 is."""
    from dexiraft_amd import _native as nat
    lib = nat.load()
    B, D, H, W, L = 2, 96, 45, 70, 4
    a1 = dg.fmap(95, B, D, H, W, "fnet")
    a2 = dg.fmap(96, B, D, H, W, "fnet")
    if case == "nonfinite":
        a1[1, 5, 10, 20] = 1.0e5
        a1[0, 3, 2, 2] = np.inf
        a2[0, 7, 30, 40] = np.nan
    ab = dx.AlternateCorrBlock(_t(a1), _t(a2), num_levels=L, radius=4)
    n = lib.dxr_alt_volume_numel(B, H, W, L, 0)
    vol = torch.full((n,), float("nan"), device=DEV)
    assert lib.dxr_alt_coarse_volumes(ab._f1_nhwc.data_ptr(), ab._f2_ptrs, B, H, W, D, L, 0,
                                      vol.data_ptr(), nat.stream_of(vol)) == 0
    # the LDS-DMA form on pre-split planes (dxr_alt_coarse_volumes_ws): the same bits
    nb = lib.dxr_alt_coarse_volumes_ws_bytes(B, H, W, D, L, 0)
    assert nb > 0
    ws = torch.empty((nb,), dtype=torch.uint8, device=DEV)
    vol_dma = torch.full((n,), float("nan"), device=DEV)
    assert lib.dxr_alt_coarse_volumes_ws(ab._f1_nhwc.data_ptr(), ab._f2_ptrs, B, H, W, D, L, 0,
                                         vol_dma.data_ptr(), ws.data_ptr(), nb,
                                         nat.stream_of(vol)) == 0
    assert torch.equal(torch.isnan(vol), torch.isnan(vol_dma))
    assert torch.equal(torch.nan_to_num(vol, nan=3.0), torch.nan_to_num(vol_dma, nan=3.0))
    N = H * W
    f1 = ab._f1_nhwc.reshape(B, N, D).double().cpu().numpy()
    with np.errstate(invalid="ignore", over="ignore"):
        for lvl in range(L):
            f2 = ab._f2_nhwc[lvl]
            h, w = f2.shape[1], f2.shape[2]
            got = torch.empty((B * N, h, w), device=DEV)
            assert lib.dxr_pyramid_unpack(vol.data_ptr(), nat.DXR_F32, B, H, W, L, lvl,
                                          got.data_ptr(), nat.stream_of(got)) == 0
            got = got.reshape(B, N, h * w).cpu().numpy()
            g2 = f2.reshape(B, h * w, D).double().cpu().numpy()
            ref = f1 @ g2.transpose(0, 2, 1)
            mag = np.abs(f1) @ np.abs(g2).transpose(0, 2, 1)
            fin = np.isfinite(ref)
            assert np.array_equal(np.isfinite(got), fin), lvl
            assert (np.abs(got[fin] - ref[fin]) <= 1e-5 * mag[fin] + 1e-30).all(), lvl
            if case == "nonfinite":
                assert not fin.all() and np.isfinite(got[1, 10 * W + 20]).all()


@pytest.mark.parametrize("levels", [4, 5])
def test_alt_volume_lookup_every_level(dx, levels):
    """dxr_alt_coarse_volumes + dxr_alt_volume_lookup from level 0 on (every
    paged level layout: 8x16 .. 1x2 tiles, and a row-major level 4) against
    dxr_alt_corr_lookup: bit for bit."""
    from dexiraft_amd import _native as nat
    lib = nat.load()
    B, D, H, W, r = 2, 64, 48, 70, 3
    f1 = _t(dg.fmap(91, B, D, H, W, "fnet"))
    f2 = _t(dg.fmap(92, B, D, H, W, "fnet"))
    ab = dx.AlternateCorrBlock(f1, f2, num_levels=levels, radius=r)
    c = _alt_flow(B, H, W, "far", 93)
    K = levels * (2 * r + 1) ** 2
    n = lib.dxr_alt_volume_numel(B, H, W, levels, 0)
    vol = torch.full((n,), float("nan"), device=DEV)
    sq = float(np.sqrt(np.float32(D)))
    assert lib.dxr_alt_coarse_volumes(ab._f1_nhwc.data_ptr(), ab._f2_ptrs, B, H, W, D, levels, 0,
                                      vol.data_ptr(), nat.stream_of(vol)) == 0
    got = torch.full((B, K, H, W), 7.0, device=DEV)
    assert lib.dxr_alt_volume_lookup(vol.data_ptr(), c.data_ptr(), got.data_ptr(), B, H, W, levels,
                                     0, r, sq, nat.stream_of(c)) == 0
    ref = torch.full((B, K, H, W), 7.0, device=DEV)
    assert lib.dxr_alt_corr_lookup(ab._f1_nhwc.data_ptr(), ab._f2_ptrs, c.data_ptr(), ref.data_ptr(),
                                   B, H, W, D, levels, r, sq, nat.stream_of(c)) == 0
    assert torch.equal(torch.nan_to_num(got, nan=3.0), torch.nan_to_num(ref, nan=3.0))


@pytest.mark.parametrize("flow", ["iid", "smooth", "far"])
@pytest.mark.parametrize("shape", [(1, 256, 55, 128, 4), (2, 64, 30, 44, 3)])
def test_alt_lookup_query_order_is_bit_identical(dx, flow, shape):
    """dxr_alt_corr_lookup_ws (AlternateCorrBlock's entry point) orders each
    level's queries first — by window position for flows that vary pixel to
    pixel, in 4 x 8 tile order for smooth ones — and must give the workspace-less
    spatial form's outputs bit for bit: the per-(cell, query) sums do not depend
    on which queries share a workgroup.  'far' mixes NaN / inf / off-image
    coordinates (the far bin) into i.i.d. flows."""
    from dexiraft_amd import _native as nat
    lib = nat.load()
    B, D, H, W, r = shape
    f1 = _t(dg.fmap(71, B, D, H, W, "fnet"))
    f2 = _t(dg.fmap(72, B, D, H, W, "fnet"))
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32),
                         indexing="ij")
    grid = np.stack([xs, ys])[None].repeat(B, 0)
    rng = np.random.default_rng(73)
    if flow == "smooth":
        u = rng.normal(0, 4, size=(B, 2, 1, 1)) + 2 * np.sin(grid / 9.0)
        c = (grid + u).astype(np.float32)
    else:
        c = (grid + rng.normal(0, 4, size=grid.shape)).astype(np.float32)
        if flow == "far":
            c[:, 0, 3, 5] = np.nan
            c[:, 1, 7, 9] = np.inf
            c[:, :, 10, 2:30:3] = -40.0
            c[:, 0, 12, :20] = 3.0e9
    ab = dx.AlternateCorrBlock(f1, f2, radius=r)
    ct = _t(np.ascontiguousarray(c))
    outs = []
    for ws in (False, True):
        out = torch.full((B, 4 * (2 * r + 1) ** 2, H, W), float("nan"), device=DEV)
        n = lib.dxr_alt_workspace_bytes(B, H, W, 4)
        buf = torch.empty(n, dtype=torch.uint8, device=DEV)
        args = (ab._f1_nhwc.data_ptr(), ab._f2_ptrs, ct.data_ptr(), out.data_ptr(), B, H, W, D, 4,
                r, float(np.sqrt(np.float32(D))))
        st = (lib.dxr_alt_corr_lookup_ws(*args, buf.data_ptr(), n, nat.stream_of(ct)) if ws
              else lib.dxr_alt_corr_lookup(*args, nat.stream_of(ct)))
        assert st == 0
        outs.append(out)
    torch.cuda.synchronize()
    assert torch.equal(torch.isnan(outs[0]), torch.isnan(outs[1]))
    fin = ~torch.isnan(outs[0])
    assert torch.equal(outs[0][fin], outs[1][fin])
    assert torch.equal(ab(ct)[fin], outs[0][fin])


def test_alt_cuda_corr_forward_ffi(dx):
    """Reference FFI form: NHWC fmaps, [B, N, H, W, 2] coords, H2 != H1."""
    B, H1, W1, H2, W2, C, N, r = 2, 9, 13, 7, 11, 64, 2, 3
    f1 = dg.normal(71, B * H1 * W1 * C).reshape(B, H1, W1, C).astype(np.float32)
    f2 = dg.normal(72, B * H2 * W2 * C).reshape(B, H2, W2, C).astype(np.float32)
    c = (dg.uniform(73, B * N * H1 * W1 * 2).reshape(B, N, H1, W1, 2) * 14 - 2).astype(np.float32)
    ref = oracle.alt_corr_forward(f1, f2, c, r, np.float64)
    (got,) = dx.alt_cuda_corr.forward(_t(f1), _t(f2), _t(c), r)
    assert tuple(got.shape) == (B, N, (2 * r + 1) ** 2, H1, W1)
    tolerance_check(got.cpu().numpy(), ref, RTOL)
    with pytest.raises(RuntimeError):
        dx.alt_cuda_corr.forward(_t(f1).transpose(1, 2), _t(f2), _t(c), r)


@pytest.mark.parametrize("C,N,r", [(300, 2, 3), (64, 1, 4), (20, 1, 0)])
def test_alt_cuda_corr_backward_ffi(dx, C, N, r):
    """alt_cuda_corr.backward vs the oracle (pinned to the forward by adjointness):
    windows partly outside fmap2, H2 != H1, C spanning two 256-channel slabs with a
    ragged tail.  fmap2_grad is summed with atomics, so the bar is the north-star
    tolerance, not bit equality."""
    B, H1, W1, H2, W2 = 2, 9, 13, 7, 11
    rd = 2 * r + 1
    f1 = dg.normal(91, B * H1 * W1 * C).reshape(B, H1, W1, C).astype(np.float32)
    f2 = dg.normal(92, B * H2 * W2 * C).reshape(B, H2, W2, C).astype(np.float32)
    c = (dg.uniform(93, B * N * H1 * W1 * 2).reshape(B, N, H1, W1, 2) * 16 - 3).astype(np.float32)
    g = dg.normal(94, B * N * rd * rd * H1 * W1).reshape(B, N, rd * rd, H1, W1).astype(np.float32)
    r1, r2, _ = oracle.alt_corr_backward(f1, f2, c, g, r)
    g1, g2, gc = dx.alt_cuda_corr.backward(_t(f1), _t(f2), _t(c), _t(g), r)
    tolerance_check(g1.cpu().numpy(), r1, RTOL)
    tolerance_check(g2.cpu().numpy(), r2, RTOL)
    assert tuple(gc.shape) == c.shape and not gc.any()
    with pytest.raises(RuntimeError):
        dx.alt_cuda_corr.backward(_t(f1), _t(f2), _t(c), _t(g[:, :, 1:]), r)


def test_alternate_block_too_small_raises_like_reference(dx):
    f1, f2 = _pair(H=15, W=40, seed=81)
    with pytest.raises(RuntimeError):
        dx.AlternateCorrBlock(f1, f2)


# --------------------------------------------------------------------------- bf16 mode
BF16_RTOL = 1e-2   # bf16 inputs + bf16 pyramid vs the f32 reference


@pytest.mark.parametrize("name", ["fnet", "ragged", "batch2_alt", "small_r3"])
def test_bf16_mode_within_its_tolerance(dx, name):
    d = load_tiny(name)
    f1, f2 = _t(d["fmap1"]).bfloat16(), _t(d["fmap2"]).bfloat16()
    cb = dx.CorrBlock(f1, f2, num_levels=d["num_levels"], radius=d["radius"])
    assert cb._buf.dtype == torch.bfloat16
    rows = torch.from_numpy(d["pyr_rows"]).to(DEV)
    for lvl in range(d["num_levels"]):
        tolerance_check(cb.corr_pyramid[lvl][rows, 0].cpu().numpy(), d[f"pyr{lvl}"], BF16_RTOL)
    # against the float64 oracle on the SAME bf16-rounded inputs only the bf16
    # storage of the pyramid (<= 2^-9 of a value) and f32 accumulation remain
    r1 = f1.float().cpu().numpy()
    r2 = f2.float().cpu().numpy()
    pyr = oracle.corr_pyramid(r1, r2, d["num_levels"], np.float64)
    for lvl in range(d["num_levels"]):
        got = cb.corr_pyramid[lvl][:, 0].cpu().numpy().astype(np.float64)
        slack = 2.0 ** -8 * np.abs(pyr[lvl]) + 1e-5 * np.nanmax(np.abs(pyr[lvl]))
        assert np.all((np.abs(got - pyr[lvl]) <= slack) | np.isnan(pyr[lvl]))
    for k in range(d["n_coords"]):
        out = cb(_t(d[f"coords{k}"]))
        tolerance_check(out.cpu().numpy(), d[f"out{k}"], BF16_RTOL)


def test_bf16_kitti_shape(dx):
    """C3 shape (47x156: partial tiles, 8-byte staging) against the reference checksums."""
    d = load_large("kitti")
    B, D, H, W, r = d["B"], d["D"], d["H"], d["W"], d["radius"]
    f1 = _t(dg.fmap(d["fmap_seeds"][0], B, D, H, W, d["dist"])).bfloat16()
    f2 = _t(dg.fmap(d["fmap_seeds"][1], B, D, H, W, d["dist"])).bfloat16()
    cb = dx.CorrBlock(f1, f2, radius=r)
    for lvl in range(4):
        a = cb.corr_pyramid[lvl].reshape(-1)
        got = a[torch.from_numpy(d[f"pyr{lvl}_idx"]).to(DEV)].cpu().numpy()
        assert np.abs(got - d[f"pyr{lvl}_val"]).max() <= BF16_RTOL * float(d[f"pyr{lvl}_maxabs"])
    mode, scale, seed = d["coords"][0]
    out = cb(_t(dg.coords(int(seed), B, H, W, mode, float(scale))))
    got = out.reshape(-1)[torch.from_numpy(d["out0_idx"]).to(DEV)].cpu().numpy()
    assert np.abs(got - d["out0_val"]).max() <= BF16_RTOL * float(d["out0_maxabs"])


@pytest.mark.parametrize("D", [256, 96])
def test_bf16_build_batched_odd_stages(dx, D):
    """bf16 build at B=3 (XCD-remapped page order across pairs) and D=96 (an odd
    number of 32-deep K stages) against the float64 oracle on the same
    bf16-rounded inputs: only the pyramid's bf16 storage rounding remains."""
    B, H, W = 3, 47, 100
    f1, f2 = _pair(B=B, D=D, H=H, W=W, seed=121, dist="fnet")
    f1, f2 = f1.bfloat16(), f2.bfloat16()
    cb = dx.CorrBlock(f1, f2)
    r1, r2 = f1.float().cpu().numpy(), f2.float().cpu().numpy()
    rows = np.random.default_rng(5).choice(B * H * W, 512, replace=False)
    n = H * W
    for lvl in range(4):
        got = cb.corr_pyramid[lvl][torch.from_numpy(rows).to(DEV), 0].cpu().numpy()
        for i, row in enumerate(rows):
            b, q = divmod(int(row), n)
            ref = oracle.corr_rows_pyramid(r1[b], r2[b], [q], lvl + 1, np.float64)[lvl][0]
            slack = 2.0 ** -8 * np.abs(ref) + 1e-5 * np.abs(ref).max()
            assert np.all(np.abs(got[i] - ref) <= slack), (lvl, row)


def test_split_build_overflow_fallback(dx):
    """Operands beyond the f16 range (|x| >= 65520) are scaled into it by the
    pre-split pass (per-pixel powers of two), so the result stays f32-class over
    the whole f32 range; non-finite operands make their pages non-finite and
    those pages are re-run on the exact-f32 MFMA, so NaN rows stay NaN, as in the
    reference's f32 matmul."""
    f1, f2 = _pair(H=24, W=32, seed=61)
    f1, f2 = f1.clone(), f2.clone()
    f1[0, :, 3, 5] *= 1.0e5                      # query (3, 5) far out of f16 range
    f2[0, 7, 10, 20] = 3.0e6                     # one target channel out of range
    cb = dx.CorrBlock(f1, f2)
    base = _build_exact_f32(f1, f2)
    for lvl in range(4):
        got, ref = cb.corr_pyramid[lvl][:, 0], base[lvl]
        assert torch.isfinite(got).all()
        assert (got - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()
    q = 3 * 32 + 5
    assert cb.corr_pyramid[0][q].abs().max().item() > 1.0e4     # the scaled row itself
    f1[0, 0, 1, 1] = float("nan")
    cb = dx.CorrBlock(f1, f2)
    lv0 = cb.corr_pyramid[0][:, 0]
    assert torch.isnan(lv0[1 * 32 + 1]).all()
    rest = torch.ones(lv0.shape[0], dtype=torch.bool, device=DEV)
    rest[1 * 32 + 1] = False
    assert torch.isfinite(lv0[rest]).all()
    assert (lv0[rest] - base[0][rest]).abs().max().item() <= 1e-5 * base[0].abs().max().item()


@pytest.mark.parametrize("big_side", ["query", "target"])
def test_prescaled_build_extreme_pixel_magnitudes(dx, big_side):
    """pixels of very different magnitudes (1e36 queries against
    1e-36 targets, and the reverse) give finite products of order one.  The
    pre-split build undoes both pixels' scales with one ldexp by the exponent
    sum, so these cells are f32-class like every other (the round-4 unscale
    multiplied by the two factors in turn and overflowed / went subnormal in
    between)."""
    H, W = 24, 32
    f1, f2 = _pair(H=H, W=W, seed=191)
    f1, f2 = f1.clone(), f2.clone()
    big, tiny = (f1, f2) if big_side == "query" else (f2, f1)
    big[0, :, 5, 9] *= 1.0e36                       # one pixel of one map ~1e36
    tiny[0, :, 11, 20] *= 1.0e-36                   # pixels of the other ~1e-36, ~1e-30
    tiny[0, :, 2, 3] *= 1.0e-30
    cb = dx.CorrBlock(f1, f2)
    r1 = f1[0].reshape(256, -1).double().cpu().numpy()
    r2 = f2[0].reshape(256, -1).double().cpu().numpy()
    ref = (r1.T @ r2) / 16.0                        # float64 level 0 [query, target]
    absref = (np.abs(r1).T @ np.abs(r2)) / 16.0     # scale of each dot product
    got = cb.corr_pyramid[0][:, 0].reshape(H * W, H * W).double().cpu().numpy()
    assert np.isfinite(got).all()
    err = np.abs(got - ref) / absref
    big_px, tiny_px = 5 * W + 9, [11 * W + 20, 2 * W + 3]
    cells = [(big_px, t) for t in tiny_px] if big_side == "query" else \
        [(q, big_px) for q in tiny_px]
    for q, t in cells:
        assert 0.1 < abs(ref[q, t]) < 1e8, (q, t, ref[q, t])    # a finite, normal product
        assert err[q, t] <= 4e-6, (q, t, got[q, t], ref[q, t])
    assert err.max() <= 4e-5


def _dma_units(B, H, W):
    """Units of the DMA build (two 128-query blocks x one 8x16 tile)."""
    qt = (H * W + 127) // 128
    return B * ((qt + 1) // 2) * ((H + 7) // 8) * ((W + 15) // 16)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_tail_quarter_units_bit_identical(dx, dtype):
    """The DMA build runs the last partial dispatch round as quarter units
    (corr_build.hip dma_grid / dma_quarter) when it is at most an eighth of a round.  A
    pair whose units fall in that tail (Sintel B=1: 1,568 units on 512 slots)
    gets the same pages bit for bit as in a batch whose grid has no tail split."""
    H, W = 55, 128
    slots = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    t1 = _dma_units(1, H, W) % slots
    if t1 == 0 or 8 * t1 > slots:
        pytest.skip("no tail split at B=1 on this device")
    b2 = next((b for b in range(2, 33) if _dma_units(b, H, W) % slots == 0 or
               8 * (_dma_units(b, H, W) % slots) > slots), None)
    if b2 is None:
        pytest.skip("no batch without a tail split")
    f1, f2 = _pair(B=b2, H=H, W=W, seed=201, dist="fnet")
    if dtype == "bf16":
        f1, f2 = f1.bfloat16(), f2.bfloat16()
    one = dx.CorrBlock(f1[:1].contiguous(), f2[:1].contiguous())
    many = dx.CorrBlock(f1, f2)
    for lvl in range(4):
        a, b = one.corr_pyramid[lvl][:, 0], many.corr_pyramid[lvl][: H * W, 0]
        assert torch.equal(torch.nan_to_num(a, nan=2.0), torch.nan_to_num(b, nan=2.0)), lvl


@pytest.mark.parametrize("W,layout", [(62, "nchw"), (32, "nhwc"), (44, "nchw")])
def test_prescaled_build_nonfinite_fallback_forms(dx, W, layout):
    """Pages that see an inf/NaN operand are recomputed from the f32 operands on
    the exact-f32 MFMA, in every operand form of that fallback (float4 / scalar
    NCHW staging, NHWC): NaN where the reference's f32 matmul has NaN,
    inf x finite = inf, and f32 class everywhere else."""
    H = 20
    f1, f2 = _pair(H=H, W=W, seed=181)
    f1, f2 = f1.clone(), f2.clone()
    f2[0, 3, 4, 5] = float("nan")                # target (4, 5): NaN for every query
    f1[0, 9, 2, 7] = float("inf")                # query (2, 7): +-inf / NaN row
    base = _build_exact_f32(f1, f2)
    if layout == "nhwc":
        f1 = f1.contiguous(memory_format=torch.channels_last)
        f2 = f2.contiguous(memory_format=torch.channels_last)
    cb = dx.CorrBlock(f1, f2)
    got, ref = cb.corr_pyramid[0][:, 0], base[0]
    assert torch.equal(torch.isnan(got), torch.isnan(ref))
    assert torch.equal(torch.isinf(got), torch.isinf(ref))
    fin = torch.isfinite(ref)
    assert (got[fin] - ref[fin]).abs().max().item() <= 1e-5 * ref[fin].abs().max().item()
    for lvl in range(1, 4):
        g, r = cb.corr_pyramid[lvl][:, 0], base[lvl]
        assert torch.equal(torch.isnan(g), torch.isnan(r)), lvl
        fin = torch.isfinite(r)
        assert (g[fin] - r[fin]).abs().max().item() <= 1e-5 * r[fin].abs().max().item(), lvl


@pytest.mark.parametrize("B,L", [(3, 4), (2, 4), (1, 2), (1, 3)])
def test_prescaled_build_nonfinite_on_whole_units(dx, B, L):
    """inf/NaN operands on the grids real inputs take.
    Sintel-size maps run whole units (B=3: 4,704 units, no tail split, so every
    page goes through the whole-unit kernel's per-wave vote and recompute); B=2
    has a 522 MB pyramid, so its pages are streamed out non-temporally (EXF 3)
    and the recompute rewrites pages that first pass wrote (its 64-unit tail
    also runs as quarter units); num_levels 2 and 3 take the vote on the
    unscaled values instead of the level-3 cells.  Each against the exact-f32
    build: NaN / inf patterns equal, f32 class elsewhere."""
    H, W = 55, 128
    f1, f2 = _pair(B=B, H=H, W=W, seed=301 + B + L, dist="fnet")
    f1, f2 = f1.clone(), f2.clone()
    for b in range(B):
        f2[b, 3 + b, 40 - b, 100 + b] = float("nan")      # a target: NaN for every query
        f1[b, 9 + b, 50 - b, 3 + 2 * b] = float("inf")    # a query: +-inf / NaN row
        f1[b, 200, 20 + b, 64] = -float("inf")
    base = _build_exact_f32(f1, f2, num_levels=L)
    cb = dx.CorrBlock(f1, f2, num_levels=L)
    for lvl in range(L):
        got, ref = cb.corr_pyramid[lvl][:, 0], base[lvl]
        assert torch.equal(torch.isnan(got), torch.isnan(ref)), lvl
        assert torch.equal(torch.isinf(got), torch.isinf(ref)), lvl
        assert torch.equal(got[torch.isinf(ref)], ref[torch.isinf(ref)]), lvl   # signs too
        fin = torch.isfinite(ref)
        assert fin.float().mean().item() > 0.95, lvl           # the pages around stay finite
        assert (got[fin] - ref[fin]).abs().max().item() <= 1e-5 * ref[fin].abs().max().item(), lvl
    del cb, base
    torch.cuda.empty_cache()


def _build_exact_f32(f1: torch.Tensor, f2: torch.Tensor, num_levels: int = 4,
                     algo: int | None = None):
    """The exact-f32 MFMA build (DXR_BUILD_EXACT_F32) through the C-ABI, as
    reference-layout levels [B*H*W, H_l, W_l] (``algo`` DXR_BUILD_AUTO: the
    workspace-less entry point's f16-pair split build of round 2)."""
    from dexiraft_amd import _native as nat
    lib = nat.load()
    B, D, H, W = (int(v) for v in f1.shape)
    buf = torch.empty(lib.dxr_pyramid_numel(B, H, W, num_levels), device=DEV)
    st = lib.dxr_corr_pyramid_build(f1.data_ptr(), f2.data_ptr(), nat.DXR_F32, nat.DXR_NCHW, B, D,
                                    H, W, num_levels, float(np.sqrt(np.float32(D))),
                                    buf.data_ptr(), nat.DXR_F32,
                                    nat.DXR_BUILD_EXACT_F32 if algo is None else algo,
                                    nat.stream_of(f1))
    assert st == 0
    out, h, w = [], H, W
    for lvl in range(num_levels):
        if lvl:
            h, w = h // 2, w // 2
        t = torch.empty((B * H * W, h, w), device=DEV)
        assert lib.dxr_pyramid_unpack(buf.data_ptr(), nat.DXR_F32, B, H, W, num_levels, lvl,
                                      t.data_ptr(), nat.stream_of(t)) == 0
        out.append(t)
    return out


def _build_no_workspace(f1, f2, num_levels=4):
    from dexiraft_amd import _native as nat
    return _build_exact_f32(f1, f2, num_levels, algo=nat.DXR_BUILD_AUTO)


@pytest.mark.parametrize("scale", [1.0, 1e-4, 1e-6, 3e3])
def test_prescaled_split_build_accuracy_is_scale_free(dx, scale):
    """the f16 pair split loses precision where a residual falls on
    f16's subnormal grid.  The default build scales each pixel by a power of two
    first, so its error relative to max|ref| does not grow as the fmaps shrink:
    within 2x the exact-f32 MFMA build's error against float64 at every scale
    (fnet-like fmaps x scale, Sintel shape)."""
    H, W = 55, 128
    f1 = (dg.fmap(151, 1, 256, H, W, "fnet") * np.float32(scale)).astype(np.float32)
    f2 = (dg.fmap(152, 1, 256, H, W, "fnet") * np.float32(scale)).astype(np.float32)
    pyr = oracle.corr_pyramid(f1, f2, 4, np.float64)
    base = _build_exact_f32(_t(f1), _t(f2))
    cb = dx.CorrBlock(_t(f1), _t(f2))
    for lvl in range(4):
        got = cb.corr_pyramid[lvl][:, 0].cpu().numpy()
        e_ws = np.abs(got - pyr[lvl]).max()
        e_mfma = np.abs(base[lvl].cpu().numpy() - pyr[lvl]).max()
        m = np.abs(pyr[lvl]).max()
        print(f"scale {scale:g} level {lvl}: max|err| pre-split {e_ws:.3e}, f32 mfma "
              f"{e_mfma:.3e}, max|ref| {m:.3e}")
        assert e_ws <= 2 * e_mfma + 1e-7 * m


def test_prescaled_build_agrees_with_workspaceless_build(dx):
    """The pre-split build (workspace) and the r02 split build (no workspace,
    dxr_corr_pyramid_build) agree to f32 rounding; NCHW and NHWC operands give
    the pre-split build's pyramid bit for bit."""
    from dexiraft_amd import _native as nat
    f1, f2 = _pair(B=2, H=30, W=44, seed=171, dist="fnet")
    ref = _build_no_workspace(f1, f2)
    cb = dx.CorrBlock(f1, f2)
    for lvl in range(4):
        a, b = cb.corr_pyramid[lvl][:, 0], ref[lvl]
        assert (a - b).abs().max().item() <= 2e-6 * b.abs().max().item(), lvl
    cl = dx.CorrBlock(f1.contiguous(memory_format=torch.channels_last),
                      f2.contiguous(memory_format=torch.channels_last))
    assert torch.equal(cb._buf, cl._buf)
    assert nat.load().dxr_build_workspace_bytes(nat.DXR_F32, 2, 256, 30, 44) > 0


@pytest.mark.parametrize("shape", [(2, 47, 156), (1, 55, 100)])
def test_split_build_agrees_with_exact_f32_build(dx, shape):
    """The default (split) build and the exact-f32 MFMA fallback agree to f32
    rounding in every valid cell.  55 x 100 has an odd number of query pages (43)
    and of target tiles per row (7): edge pages are partly padding."""
    B, H, W = shape
    f1, f2 = _pair(B=B, H=H, W=W, seed=111, dist="fnet")
    ref = _build_exact_f32(f1, f2)
    cb = dx.CorrBlock(f1, f2)
    for lvl in range(4):
        a, b = cb.corr_pyramid[lvl][:, 0], ref[lvl]
        scale = b.abs().max().item()
        assert (a - b).abs().max().item() <= 2e-6 * scale, f"level {lvl}"


def test_split_build_f32_accuracy(dx):
    """The split build (f32 operands as f16 pairs hi + 2^-11 lo, three f16 MFMA
    products into two f32 accumulators) has f32-class error: within RTOL of the
    float64 oracle everywhere, and no worse than 2x the f32-MFMA build's own error."""
    H, W = 55, 128
    f1 = dg.fmap(51, 1, 256, H, W, "fnet")
    f2 = dg.fmap(52, 1, 256, H, W, "fnet")
    c = dg.coords(53, 1, H, W, "normal", 4.0)
    pyr = oracle.corr_pyramid(f1, f2, 4, np.float64)
    base = _build_exact_f32(_t(f1), _t(f2))
    cb = dx.CorrBlock(_t(f1), _t(f2))
    for lvl in range(4):
        got = cb.corr_pyramid[lvl][:, 0].cpu().numpy()
        tolerance_check(got, pyr[lvl], RTOL)
        e_split = np.abs(got - pyr[lvl]).max()
        e_mfma = np.abs(base[lvl].cpu().numpy() - pyr[lvl]).max()
        print(f"level {lvl}: max|err| split {e_split:.3e}, f32 mfma {e_mfma:.3e}, "
              f"max|ref| {np.abs(pyr[lvl]).max():.2f}")
        assert e_split <= 2 * e_mfma + 1e-6
    tolerance_check(cb(_t(c)).cpu().numpy(), oracle.corr_lookup(pyr, c, 4), RTOL)
    for name in ("nanlevel", "batch2_alt", "min8"):          # D % 16 == 0, W % 4 == 0
        d = load_tiny(name)
        cb = dx.CorrBlock(_t(d["fmap1"]), _t(d["fmap2"]), num_levels=d["num_levels"],
                          radius=d["radius"])
        rows = torch.from_numpy(d["pyr_rows"]).to(DEV)
        for lvl in range(d["num_levels"]):
            tolerance_check(cb.corr_pyramid[lvl][rows, 0].cpu().numpy(), d[f"pyr{lvl}"], RTOL)
        for k in range(d["n_coords"]):
            tolerance_check(cb(_t(d[f"coords{k}"])).cpu().numpy(), d[f"out{k}"], RTOL)


# --------------------------------------------------------------------------- edge cases / API
def test_empty_batch(dx):
    f = torch.empty((0, 256, 20, 24), device=DEV)
    cb = dx.CorrBlock(f, f)
    out = cb(torch.empty((0, 2, 20, 24), device=DEV))
    assert tuple(out.shape) == (0, 324, 20, 24)


def test_too_small_fmap_raises(dx):
    f1, f2 = _pair(H=7, W=30, seed=91)
    with pytest.raises(RuntimeError):
        dx.CorrBlock(f1, f2)          # level 3 of a 7-row map is empty
    cb = dx.CorrBlock(f1, f2, num_levels=3)  # 7 -> 3 -> 1: fine
    assert cb.corr_pyramid[2].shape[-2:] == (1, 7)


def test_noncontiguous_inputs(dx):
    f1, f2 = _pair(H=24, W=30, seed=93)
    c = _t(dg.coords(94, 1, 24, 30, "normal", 3.0))
    ref = dx.CorrBlock(f1, f2)(c)
    g1 = f1.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    cnc = c.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not g1.is_contiguous() and not cnc.is_contiguous()
    assert torch.equal(dx.CorrBlock(g1, f2)(cnc), ref)


def test_radius_and_levels_variants(dx):
    H, W = 32, 40
    f1 = dg.fmap(95, 1, 64, H, W)
    f2 = dg.fmap(96, 1, 64, H, W)
    c = dg.coords(97, 1, H, W, "normal", 3.0)
    for L, r in ((1, 0), (2, 2), (4, 6), (6, 1)):
        pyr = oracle.corr_pyramid(f1, f2, L, np.float64)
        ref = oracle.corr_lookup(pyr, c, r)
        got = dx.CorrBlock(_t(f1), _t(f2), num_levels=L, radius=r)(_t(c)).cpu().numpy()
        tolerance_check(got, ref, RTOL)


def test_grad_inputs_without_a_backward_raise(dx):
    """Autograd is supported for f32 CorrBlock only (§3.5): bf16 fmaps and the
    alternate block raise loudly when their inputs require grad."""
    f1, f2 = _pair(H=16, W=16, seed=98)
    f1.requires_grad_(True)
    dx.CorrBlock(f1, f2)                                    # differentiable
    with pytest.raises(NotImplementedError):
        dx.CorrBlock(f1.bfloat16(), f2.bfloat16())
    with pytest.raises(NotImplementedError):
        dx.AlternateCorrBlock(f1, f2, num_levels=3)
    with torch.no_grad():
        dx.CorrBlock(f1.bfloat16(), f2.bfloat16())
        dx.AlternateCorrBlock(f1, f2, num_levels=3)


def test_bad_coords_shape_raises(dx):
    f1, f2 = _pair(H=16, W=16, seed=99)
    cb = dx.CorrBlock(f1, f2)
    with pytest.raises(RuntimeError):
        cb(torch.zeros((1, 2, 16, 15), device=DEV))


def test_side_stream(dx):
    f1, f2 = _pair(H=30, W=40, seed=101)
    c = _t(dg.coords(102, 1, 30, 40, "normal", 3.0))
    ref = dx.CorrBlock(f1, f2)(c)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = dx.CorrBlock(f1, f2)(c)
    torch.cuda.current_stream().wait_stream(s)
    assert torch.equal(out, ref)


def test_corr_pyramid_is_cached_reference_layout(dx):
    f1, f2 = _pair(H=19, W=37, seed=103)
    cb = dx.CorrBlock(f1, f2)
    p = cb.corr_pyramid
    assert p is cb.corr_pyramid
    assert [tuple(t.shape) for t in p] == [(703, 1, 19, 37), (703, 1, 9, 18), (703, 1, 4, 9),
                                           (703, 1, 2, 4)]
    assert all(t.is_contiguous() and t.dtype == torch.float32 for t in p)


def test_native_library_is_the_one_loaded(dx):
    """The in-tree .so is mapped into this process (no silent fallback)."""
    maps = open("/proc/self/maps").read()
    assert str(dx.LIB_PATH) in maps


# --------------------------------------------------------------------------- backward
BW_RTOL = 1e-4   # of max|reference gradient|, as the forward's fp32 tolerance


def _loss_backward(block_cls, f1, f2, coord_sets, weights, **kw):
    f1 = f1.clone().requires_grad_(True)
    f2 = f2.clone().requires_grad_(True)
    cb = block_cls(f1, f2, **kw)
    loss = 0.0
    for c, w in zip(coord_sets, weights):
        loss = loss + (cb(c) * w).sum()
    loss.backward()
    return f1.grad, f2.grad


def test_training_step_frees_memory_without_gc(dx):
    """A differentiable block (pyramid + gradient pyramid, hundreds of MB at
    benchmark sizes) is freed by refcount when the step's tensors go: the
    autograd nodes hold only the block's _GradState, never the block, so no
    reference cycle waits for Python's cyclic collector."""
    import gc
    f1, f2 = _pair(H=30, W=44, seed=41)
    c = [_t(dg.coords(42 + k, 1, 30, 44, "normal", 3.0)) for k in range(3)]

    def one_step():
        a1, a2 = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
        cb = dx.CorrBlock(a1, a2)
        sum(cb(ci).sum() for ci in c).backward()

    one_step()          # first GEMM: torch's persistent BLAS workspace comes from the allocator
    torch.cuda.synchronize()
    gc.collect()
    base = torch.cuda.memory_allocated()
    gc.disable()
    try:
        for _ in range(3):
            a1, a2 = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
            cb = dx.CorrBlock(a1, a2)
            loss = sum(cb(ci).sum() for ci in c)
            loss.backward()
            assert a1.grad is not None and a2.grad is not None
            del a1, a2, cb, loss
            torch.cuda.synchronize()
            assert torch.cuda.memory_allocated() == base
    finally:
        gc.enable()


@pytest.mark.parametrize("name", ["bw_basic", "bw_batch2_r3", "bw_d256"])
def test_backward_matches_reference_autograd_golden(dx, name):
    """d loss / d fmaps through CorrBlock (build + 3 lookups) against the
    reference's own autograd gradients (tests/golden/make_backward_golden.py)."""
    from conftest import load_backward
    d = load_backward(name)
    g1, g2 = _loss_backward(dx.CorrBlock, _t(d["fmap1"]), _t(d["fmap2"]),
                            [_t(c) for c in d["coords"]], [_t(w) for w in d["weights"]],
                            num_levels=d["num_levels"], radius=d["radius"])
    for got, ref in ((g1, d["dfmap1"]), (g2, d["dfmap2"])):
        scale = np.abs(ref).max()
        err = np.abs(got.cpu().numpy() - ref).max()
        print(f"{name}: max|err| {err:.3e} of max|grad| {scale:.3e}")
        assert err <= BW_RTOL * scale


@pytest.mark.parametrize("shape", [(1, 256, 46, 62, 4), (2, 128, 23, 37, 3)])
def test_backward_matches_torch_autograd(dx, shape):
    """Chairs-size and a ragged batch-2 case against torch autograd of the
    PyTorch restatement (tests/torch_ref.py) on the same device, 12 lookups."""
    from torch_ref import TorchCorrBlock
    B, D, H, W, r = shape
    f1, f2 = _pair(B=B, D=D, H=H, W=W, seed=301, dist="fnet")
    cs = [_t(dg.coords(310 + k, B, H, W, "normal", 4.0)) for k in range(12)]
    ws = [_t(dg.fmap(330 + k, B, 4 * (2 * r + 1) ** 2, H, W)) for k in range(12)]
    g1, g2 = _loss_backward(dx.CorrBlock, f1, f2, cs, ws, radius=r)
    t1, t2 = _loss_backward(TorchCorrBlock, f1, f2, cs, ws, radius=r)
    for got, ref in ((g1, t1), (g2, t2)):
        scale = ref.abs().max().item()
        err = (got - ref).abs().max().item()
        print(f"{shape}: max|err| {err:.3e} of max|grad| {scale:.3e}")
        assert err <= BW_RTOL * scale


def test_backward_of_static_corr(dx):
    """CorrBlock.corr is differentiable (core/corr.py:52-60 is a plain matmul)."""
    f1, f2 = _pair(B=2, D=64, H=12, W=20, seed=341)
    w = _t(dg.fmap(342, 2 * 12 * 20, 1, 12 * 20, 1)).reshape(2, 12, 20, 1, 12, 20)
    a1, a2 = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
    (dx.CorrBlock.corr(a1, a2) * w).sum().backward()
    b1, b2 = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
    v = torch.bmm(b1.reshape(2, 64, -1).transpose(1, 2), b2.reshape(2, 64, -1)) / 8.0
    (v.reshape(2, 12, 20, 1, 12, 20) * w).sum().backward()
    for got, ref in ((a1.grad, b1.grad), (a2.grad, b2.grad)):
        assert (got - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()


def test_split_build_even_width_not_multiple_of_4(dx):
    """Chairs' 62-wide fmaps take the split build with float2 target units: f32
    class against the float64 oracle, and no worse than the exact-f32 MFMA build."""
    H, W = 46, 62
    f1 = dg.fmap(61, 1, 256, H, W, "fnet")
    f2 = dg.fmap(62, 1, 256, H, W, "fnet")
    pyr = oracle.corr_pyramid(f1, f2, 4, np.float64)
    base = _build_exact_f32(_t(f1), _t(f2))
    cb = dx.CorrBlock(_t(f1), _t(f2))
    for lvl in range(4):
        got = cb.corr_pyramid[lvl][:, 0].cpu().numpy()
        tolerance_check(got, pyr[lvl], RTOL)
        e_split = np.abs(got - pyr[lvl]).max()
        e_mfma = np.abs(base[lvl].cpu().numpy() - pyr[lvl]).max()
        assert e_split <= 2 * e_mfma + 1e-6


def test_backward_only_flows_to_fmaps_that_require_grad(dx):
    f1, f2 = _pair(B=1, D=32, H=12, W=16, seed=351)
    a1 = f1.clone().requires_grad_(True)
    cb = dx.CorrBlock(a1, f2)
    c = _t(dg.coords(352, 1, 12, 16, "normal", 2.0))
    cb(c).sum().backward()
    assert a1.grad is not None and torch.isfinite(a1.grad).all()
    with torch.no_grad():                       # inference calls on a grad block stay plain
        out = cb(c)
    assert out.grad_fn is None
    with pytest.raises(NotImplementedError, match="coords"):
        cb(c.clone().requires_grad_(True))


# Every build kernel the library can run, by the request that selects it
# (include/dexiraft_corr.h, "Kernels by request"): the test id names the kernel
# that request reaches — tests/test_build_plan.py checks which kernel it is, on
# a CPU, against the planner (csrc/build_plan.h).  Each runs through the C-ABI
# and is checked against the float64 oracle at the dtype's tolerance (f32 1e-4
# of max per level, bf16 1e-2).
_BUILD_PATHS = [
    # id, in dtype, layout, workspace, algo, (B, D, H, W)
    ("split_pairs_kernel+corr_build_dma_kernel", "f32", "nchw", True, "auto", (1, 64, 23, 31)),
    ("split_pairs_kernel+corr_build_dma_kernel-nhwc", "f32", "nhwc", True, "auto", (1, 64, 23, 32)),
    ("corr_build_split_kernel", "f32", "nchw", False, "auto", (1, 64, 23, 32)),
    ("corr_build_split_kernel-nhwc", "f32", "nhwc", False, "auto", (1, 64, 23, 32)),
    ("corr_build_f32_kernel-exact", "f32", "nchw", False, "exact", (1, 64, 23, 32)),
    ("corr_build_f32_kernel-exact-ws", "f32", "nchw", True, "exact", (1, 64, 23, 32)),
    ("corr_build_f32_kernel-d24", "f32", "nchw", True, "auto", (1, 24, 23, 31)),
    ("pack_bf16_kernel+corr_build_dma_kernel", "bf16", "nchw", True, "auto", (1, 64, 23, 32)),
    ("corr_build_dma_kernel-bf16-nhwc", "bf16", "nhwc", False, "auto", (1, 64, 23, 32)),
    ("corr_build_bf16_q2_kernel", "bf16", "nchw", False, "auto", (1, 64, 23, 32)),
    ("corr_build_bf16_kernel-w31", "bf16", "nchw", False, "auto", (1, 64, 23, 31)),
]


@pytest.mark.parametrize("path", _BUILD_PATHS, ids=[p[0] for p in _BUILD_PATHS])
def test_build_kernel_by_request(dx, path):
    from dexiraft_amd import _native as nat
    _, dt, layout, with_ws, algo, (B, D, H, W) = path
    lib = nat.load()
    a = dg.fmap(881, B, D, H, W, "fnet")
    b = dg.fmap(882, B, D, H, W, "fnet")
    ref = oracle.corr_pyramid(a, b, 4, np.float64)
    f1, f2 = _t(a), _t(b)
    code = nat.DXR_F32
    if dt == "bf16":
        f1, f2, code = f1.bfloat16(), f2.bfloat16(), nat.DXR_BF16
        ref = oracle.corr_pyramid(f1.float().cpu().numpy(), f2.float().cpu().numpy(), 4, np.float64)
    lay = nat.DXR_NCHW
    if layout == "nhwc":
        f1 = f1.contiguous(memory_format=torch.channels_last)
        f2 = f2.contiguous(memory_format=torch.channels_last)
        lay = nat.DXR_NHWC
    buf = torch.empty(lib.dxr_pyramid_numel(B, H, W, 4), device=DEV,
                      dtype=torch.float32 if dt == "f32" else torch.bfloat16)
    al = nat.DXR_BUILD_EXACT_F32 if algo == "exact" else nat.DXR_BUILD_AUTO
    div = float(np.sqrt(np.float32(D)))
    s = nat.stream_of(f1)
    if with_ws:
        nb = max(lib.dxr_build_workspace_bytes(code, B, D, H, W), 0)
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=DEV)
        st = lib.dxr_corr_pyramid_build_ws(f1.data_ptr(), f2.data_ptr(), code, lay, B, D, H, W, 4,
                                           div, buf.data_ptr(), code, al, ws.data_ptr(), nb, s)
    else:
        st = lib.dxr_corr_pyramid_build(f1.data_ptr(), f2.data_ptr(), code, lay, B, D, H, W, 4, div,
                                        buf.data_ptr(), code, al, s)
    assert st == 0
    tol = 1e-4 if dt == "f32" else 1e-2
    h, w = H, W
    for lvl in range(4):
        if lvl:
            h, w = h // 2, w // 2
        t = torch.empty((B * H * W, h, w), device=DEV)
        assert lib.dxr_pyramid_unpack(buf.data_ptr(), code, B, H, W, 4, lvl, t.data_ptr(), s) == 0
        got = t.cpu().numpy()
        m = np.abs(ref[lvl]).max()
        assert np.abs(got - ref[lvl].reshape(got.shape)).max() <= tol * m, lvl
