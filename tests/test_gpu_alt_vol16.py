"""GPU: float16 coarse volumes of the alternate block (DXR_ALT_VOL_F16;
``AlternateCorrBlock(..., volume_dtype=torch.float16)``).

No new tolerance is involved.  The definition is two bit-equalities:

  - the float16 buffer the volume GEMM stores is ``vol32.half()`` of the float32
    buffer of the same request, element for element (to nearest even, beyond
    65504 to +-inf, subnormals kept), in its register form and its LDS-DMA form;
  - a lookup on float16 volumes is the float32-volume lookup of ``vol16.float()``
    with the same output flags, NaNs in equal places and equal bits elsewhere.

The class is held to the same two through its public interface, and one derived
bound compares it with the block's own float32 volumes: per coarse level l and
pair, |delta| <= ((2^-11 + 2^-21) Vmax_l + 2^-25) / sqrt(D), Vmax_l the level's
largest |cell| — half a float16 ulp of a normal cell or the subnormal step
2^-25 per cell, bilinear weights that are non-negative and sum to at most 1, and
2^-21 Vmax_l for the float32 arithmetic of the four taps on either side.

Shapes are the smallest at which the kernels can go wrong: 48 x 70 from level 0
has all four tile shapes (T = 128, 32, 8, 2), ragged level edges, a partial last
query page and two pairs; the lookups run both launch shapes (r <= 4 on few and
on many workgroups, r > 4).
"""
from __future__ import annotations

import ctypes
from functools import lru_cache

import numpy as np
import pytest
import torch

import datagen as dg

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
VOL16, F16, BF16, NHWC = 0x40000, 0x100, 0x200, 0x1000
OUT_FLAGS = (0, F16, BF16, NHWC, NHWC | F16, NHWC | BF16)
SENTINEL = 1.5   # exact in float16 and bfloat16


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
    return torch.from_numpy(np.array(a)).to(DEV)


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def assert_same(got: torch.Tensor, want: torch.Tensor, tag: str) -> None:
    """NaNs in equal places, equal bits elsewhere."""
    assert got.dtype == want.dtype and got.shape == want.shape, tag
    ng, nw = torch.isnan(got), torch.isnan(want)
    assert torch.equal(ng, nw), f"{tag}: NaN positions differ"
    bad = (_bits(got) != _bits(want)) & ~ng
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{tag}: {int(bad.sum())} of {bad.numel()} elements differ, first at "
                             f"{i}: got {got.flatten()[i].item()!r} want {want.flatten()[i].item()!r}")


def _flow(B, H, W, kind, seed):
    """The pixel grid + N(0, 4); far: NaN, inf, -40 and 3e9 among them (the set of
    tests/test_gpu_parity.py's coarse-volume test)."""
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32),
                         indexing="ij")
    grid = np.stack([xs, ys])[None].repeat(B, 0)
    c = (grid + np.random.default_rng(seed).normal(0, 4, size=grid.shape)).astype(np.float32)
    if kind == "far":
        c[:, 0, 3, 5] = np.nan
        c[:, 1, 7, 9] = np.inf
        c[:, :, 10, 2:30:3] = -40.0
        c[:, 0, 12, :20] = 3.0e9
    return _t(np.ascontiguousarray(c))


# --------------------------------------------------------------------------- the volume GEMM
GEMM_SHAPES = {"d64": (2, 64, 48, 70, 4), "d96": (2, 96, 45, 70, 4)}


@lru_cache(maxsize=2)
def _fmaps(shape: str):
    B, D, H, W, L = GEMM_SHAPES[shape]
    a = tuple(dg.fmap(700 + 10 * len(shape) + D + k, B, D, H, W, "fnet") for k in (1, 2))
    for x in a:
        x.flags.writeable = False
    return a


def _volumes(dx, shape, a1, a2, flag, ws):
    """The volumes of every level (first_level 0) into a zero-filled buffer."""
    nat = _nat()
    lib = nat.load()
    B, D, H, W, L = GEMM_SHAPES[shape]
    ab = dx.AlternateCorrBlock(_t(a1), _t(a2), num_levels=L, radius=4)
    assert ab._f1_nhwc.dtype == torch.float32 and ab.coarse_first_level is None
    n = lib.dxr_alt_volume_numel(B, H, W, L, 0)
    vol = torch.zeros((n,), dtype=torch.float16 if flag else torch.float32, device=DEV)
    assert vol.data_ptr() % 16 == 0
    args = (ab._f1_nhwc.data_ptr(), ab._f2_ptrs, B, H, W, D, L, flag, vol.data_ptr())
    if ws:
        nb = lib.dxr_alt_coarse_volumes_ws_bytes(B, H, W, D, L, 0)
        assert nb > 0
        w = torch.empty(nb, dtype=torch.uint8, device=DEV)
        st = lib.dxr_alt_coarse_volumes_ws(*args, w.data_ptr(), nb, nat.stream_of(vol))
    else:
        st = lib.dxr_alt_coarse_volumes(*args, nat.stream_of(vol))
    nat.check(st, f"volumes {shape} flag={flag:#x} ws={ws}")
    torch.cuda.synchronize()
    return vol


@lru_cache(maxsize=2)
def _ref32(shape: str):
    """The float32 volumes of the unscaled fmaps (register form): computed once."""
    import dexiraft_amd
    a1, a2 = _fmaps(shape)
    return _volumes(dexiraft_amd, shape, a1, a2, 0, False)


def _check_buffer(dx, shape, a1, a2, populated=None):
    ref = _volumes(dx, shape, a1, a2, 0, False)
    if populated is not None:
        assert populated(ref), "the float32 reference does not populate the range under test"
    want = ref.half()
    for ws in (False, True):
        got = _volumes(dx, shape, a1, a2, VOL16, ws)
        assert got.dtype == torch.float16 and got.numel() == ref.numel()
        assert_same(got, want, f"{shape} ws={ws}")
    return ref


@pytest.mark.parametrize("shape", list(GEMM_SHAPES))
def test_buffer_is_the_float32_buffer_rounded_once(dx, shape):
    a1, a2 = _fmaps(shape)
    ref = _check_buffer(dx, shape, a1, a2)
    assert torch.isfinite(ref).all() and bool((ref != 0).any())
    assert torch.equal(ref, _ref32(shape))


def _pow2_scale(shape: str, target: float) -> float:
    """The power of two that takes the unscaled volumes' largest |cell| into
    [target, 2 target): chosen from the float32 reference, an input of the test."""
    m = float(_ref32(shape).abs().max())
    assert m > 0
    return float(2.0 ** np.ceil(np.log2(target / m)))


def _scaled(shape: str, s: float):
    """Both fmaps scaled by powers of two whose product is s (exact)."""
    a1, a2 = _fmaps(shape)
    e = int(np.log2(s))
    return (a1 * np.float32(2.0 ** (e // 2))).astype(np.float32), \
        (a2 * np.float32(2.0 ** (e - e // 2))).astype(np.float32)


def test_cells_beyond_float16s_range_become_inf(dx):
    """The largest |cell| at 4-8 x 65504: finite float32 sums that round to +-inf
    are stored as +-inf (and do not send their tile to the fallback: the buffer
    is still the float32 buffer's .half())."""
    a1, a2 = _scaled("d64", _pow2_scale("d64", 4 * 65504.0))

    def populated(ref):
        fin = torch.isfinite(ref)
        return bool(fin.all()) and bool((ref > 65504).any()) and bool((ref < -65504).any()) and \
            bool(((ref.abs() < 65504) & (ref != 0)).any())

    ref = _check_buffer(dx, "d64", a1, a2, populated)
    assert bool(torch.isinf(ref.half()).any())


def test_small_cells_land_on_the_subnormal_grid(dx):
    """The largest |cell| at 2^-13..2^-12: most cells below 2^-14."""
    a1, a2 = _scaled("d64", _pow2_scale("d64", 2.0 ** -13))

    def populated(ref):
        m = ref.abs()
        return bool(((m < 2.0 ** -14) & (m > 2.0 ** -24)).any()) and bool((m >= 2.0 ** -14).any()) \
            and bool(((m < 2.0 ** -25) & (m > 0)).any())

    ref = _check_buffer(dx, "d64", a1, a2, populated)
    h = ref.half()
    assert bool(((h != 0) & (h.abs() < 2.0 ** -14)).any())


def test_nonfinite_operands_and_the_fallback_tile(dx):
    """A NaN fmap2 pixel, an inf fmap1 pixel and a channel of 1e5 (its tiles re-run
    on the bf16 split): NaNs in equal places, equal bits elsewhere."""
    a1, a2 = (np.array(a) for a in _fmaps("d96"))
    a1[1, 5, 10, 20] = 1.0e5
    a1[0, 3, 2, 2] = np.inf
    a2[0, 7, 30, 40] = np.nan
    ref = _check_buffer(dx, "d96", a1, a2,
                        lambda r: bool(torch.isnan(r).any()) and bool(torch.isinf(r).any()))
    assert bool(torch.isfinite(ref).any())


# --------------------------------------------------------------------------- the volume lookup
def _lookup(vol, c, geom, r, flags, first):
    """dxr_alt_volume_lookup into a sentinel-filled buffer of the flags' dtype;
    returns the whole flat buffer (channels of levels below `first` keep the
    sentinel)."""
    nat = _nat()
    B, D, H, W, L = geom
    dt = torch.float16 if flags & F16 else torch.bfloat16 if flags & BF16 else torch.float32
    out = torch.full((B * L * (2 * r + 1) ** 2 * H * W + 64,), SENTINEL, dtype=dt, device=DEV)
    st = nat.load().dxr_alt_volume_lookup(vol.data_ptr(), c.data_ptr(), out.data_ptr(), B, H, W, L,
                                          first, r | flags, float(np.sqrt(np.float32(D))),
                                          nat.stream_of(out))
    nat.check(st, f"volume lookup r={r} flags={flags:#x}")
    torch.cuda.synchronize()
    return out


LOOKUP_RUNS = [(r, 0) for r in (0, 3, 4, 5, 6, 8)] + [(4, f) for f in OUT_FLAGS[1:]] + \
    [(6, NHWC | F16), (6, BF16)]


@pytest.mark.parametrize("r,flags", LOOKUP_RUNS, ids=[f"r{r}-{f:#x}" for r, f in LOOKUP_RUNS])
def test_lookup_is_the_float32_lookup_of_the_widened_volume(dx, r, flags):
    """On the GEMM's own float16 volumes of every level (all four tile shapes);
    few workgroups: the 256-thread shape for r <= 4, the 512-thread one above."""
    geom = GEMM_SHAPES["d64"]
    B, D, H, W, L = geom
    a1, a2 = _fmaps("d64")
    vol16 = _vol16_d64(dx)
    wide = vol16.float()
    for kind in ("iid", "far"):
        c = _flow(B, H, W, kind, 71)
        got = _lookup(vol16, c, geom, r, flags | VOL16, 0)
        want = _lookup(wide, c, geom, r, flags, 0)
        assert_same(got, want, f"r={r} flags={flags:#x} {kind}")
        assert bool(torch.isnan(want.float()).any()) == (kind == "far")
        assert bool(((want.float() != SENTINEL) & (want.float() != 0)).any())


_VOL16 = {}


def _vol16_d64(dx):
    if "d64" not in _VOL16:
        a1, a2 = _fmaps("d64")
        _VOL16["d64"] = _volumes(dx, "d64", a1, a2, VOL16, False)
    return _VOL16["d64"]


@pytest.mark.parametrize("r,flags", [(4, 0), (3, NHWC | F16), (2, BF16)])
def test_lookup_on_many_workgroups_and_every_kind_of_cell(dx, r, flags):
    """More than 1024 workgroups of 32 queries: the 512-thread shape for r <= 4.
    The volumes (levels 1-3 of four pairs) are random float16 cells with +-inf,
    NaN, subnormal and zero cells among them."""
    geom = (4, 64, 48, 70, 4)
    B, D, H, W, L = geom
    assert -(-H * W // 32) * 3 * B > 1024
    n = _nat().load().dxr_alt_volume_numel(B, H, W, L, 1)
    g = torch.Generator(device=DEV).manual_seed(5)
    vol16 = (torch.randn(n, device=DEV, generator=g) * 40).half()
    k = torch.arange(n, device=DEV)
    vol16[k % 97 == 3] = float("inf")
    vol16[k % 101 == 5] = float("-inf")
    vol16[k % 103 == 7] = float("nan")
    vol16[k % 11 == 1] *= 2.0 ** -20   # subnormal
    vol16[k % 13 == 2] = 0
    assert bool(((vol16 != 0) & (vol16.abs() < 2.0 ** -14)).any())
    wide = vol16.float()
    for kind in ("iid", "far"):
        c = _flow(B, H, W, kind, 72)
        got = _lookup(vol16, c, geom, r, flags | VOL16, 1)
        want = _lookup(wide, c, geom, r, flags, 1)
        assert_same(got, want, f"many r={r} flags={flags:#x} {kind}")
        assert bool(torch.isinf(want.float()).any()) and bool(torch.isnan(want.float()).any())


# --------------------------------------------------------------------------- the class
CLASS_SHAPES = [(1, 256, 55, 128, 4), (2, 64, 30, 44, 3)]


def _force_volumes(dx, monkeypatch, max_cells=1 << 20):
    monkeypatch.setattr(dx.AlternateCorrBlock, "COARSE_MIN_QUERIES", 0)
    monkeypatch.setattr(dx.AlternateCorrBlock, "COARSE_LEVEL_MAX_CELLS", max_cells)
    monkeypatch.setattr(dx.AlternateCorrBlock, "COARSE_VOLUME_MAX_BYTES", 1 << 32)


def _class_fmaps(B, D, H, W, dtype):
    f1 = _t(dg.fmap(81, B, D, H, W, "fnet")).to(dtype)
    f2 = _t(dg.fmap(82, B, D, H, W, "fnet")).to(dtype)
    return f1, f2


def _check_block(dx, f1, f2, L, r, first, kinds, cls=None):
    """volume_dtype=torch.float16 against the float32-volume block whose volumes
    are .half().float() of themselves."""
    cls = cls or dx.AlternateCorrBlock
    B, D, H, W = f1.shape
    for kw in kinds:
        b16 = cls(f1, f2, L, r, volume_dtype=torch.float16, **kw)
        b32 = dx.AlternateCorrBlock(f1, f2, L, r, volume_dtype=torch.float32, **kw)
        assert b16.coarse_first_level == b32.coarse_first_level == first
        assert b16._volumes.dtype == torch.float16 and b16.volume_dtype == torch.float16
        assert b32._volumes.dtype == torch.float32 and b32.volume_dtype == torch.float32
        assert b16._volumes.numel() == b32._volumes.numel() == \
            _nat().load().dxr_alt_volume_numel(B, H, W, L, first)
        b32._volumes = b32._volumes.half().float()
        for kind in ("iid", "far"):
            c = _flow(B, H, W, kind, 83)
            got, want = b16(c), b32(c)
            assert got.stride() == want.stride()
            assert_same(got, want, f"{tuple(f1.shape)} {f1.dtype} {kw} {kind}")
    return b16


KINDS = ({}, {"out_dtype": torch.float16, "memory_format": torch.channels_last})


@pytest.mark.parametrize("fdt", [torch.float32, torch.float16, torch.bfloat16],
                         ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("shape", CLASS_SHAPES, ids=["d256", "d64"])
def test_block_with_float16_volumes(dx, shape, fdt, monkeypatch):
    B, D, H, W, r = shape
    _force_volumes(dx, monkeypatch)
    f1, f2 = _class_fmaps(B, D, H, W, fdt)
    b16 = _check_block(dx, f1, f2, 4, r, 1, KINDS)
    assert b16._in16 == (fdt == torch.float16) and b16._inbf16 == (fdt == torch.bfloat16)
    # the buffer itself: the float32 block's, rounded once
    b32 = dx.AlternateCorrBlock(f1, f2, 4, r)
    assert b32.volume_dtype == torch.float32
    assert_same(b16._volumes, b32._volumes.half(), "class buffer")


@pytest.mark.parametrize("shape", CLASS_SHAPES, ids=["d256", "d64"])
def test_derived_bound_against_the_float32_volume_block(dx, shape, monkeypatch):
    B, D, H, W, r = shape
    L, first, k = 4, 1, (2 * r + 1) ** 2
    _force_volumes(dx, monkeypatch)
    f1, f2 = _class_fmaps(B, D, H, W, torch.float32)
    b16 = dx.AlternateCorrBlock(f1, f2, L, r, volume_dtype=torch.float16)
    b32 = dx.AlternateCorrBlock(f1, f2, L, r)
    assert b16.coarse_first_level == b32.coarse_first_level == first
    lib = _nat().load()
    off = [lib.dxr_pyramid_level_offset(B, H, W, l) for l in range(L)] + \
        [lib.dxr_pyramid_numel(B, H, W, L)]
    c = _flow(B, H, W, "iid", 84)
    a, b = b16(c).double(), b32(c).double()
    assert torch.isfinite(b).all()
    assert torch.equal(_bits(b16(c)[:, :first * k]), _bits(b32(c)[:, :first * k])), "fine levels"
    for l in range(first, L):
        lev = b32._volumes[off[l] - off[first]:off[l + 1] - off[first]].view(B, -1)   # pair-major
        vmax = lev.abs().amax(dim=1).double()
        assert bool((vmax > 0).all()) and bool((vmax < 65504).all())
        bound = ((2.0 ** -11 + 2.0 ** -21) * vmax + 2.0 ** -25) / float(np.sqrt(np.float64(D)))
        d = (a[:, l * k:(l + 1) * k] - b[:, l * k:(l + 1) * k]).abs().amax(dim=(1, 2, 3))
        print(f"level {l}: max |delta| {d.tolist()} bound {bound.tolist()}")
        assert bool((d <= bound).all()), (l, d.tolist(), bound.tolist())
        assert bool((d > 0).any()), "the float16 volumes changed nothing: a vacuous bound"


def test_unserved_shapes_fall_back_to_rounding_the_float32_volumes(dx, monkeypatch):
    # D = 48: the levels take the FULL box form, which stores float32
    _force_volumes(dx, monkeypatch)
    f1, f2 = _class_fmaps(2, 48, 30, 44, torch.float32)
    _check_block(dx, f1, f2, 4, 3, 1, KINDS)
    # 5 levels, volumes from level 2: level 4 is row-major
    _force_volumes(dx, monkeypatch, max_cells=500)
    f1, f2 = _class_fmaps(1, 64, 55, 128, torch.float32)
    _check_block(dx, f1, f2, 5, 4, 2, KINDS[:1])


def test_block_without_volumes_ignores_the_argument(dx):
    B, D, H, W = 2, 64, 30, 44
    assert H * W < dx.AlternateCorrBlock.COARSE_MIN_QUERIES
    f1, f2 = _class_fmaps(B, D, H, W, torch.float32)
    blk = dx.AlternateCorrBlock(f1, f2, 4, 3, volume_dtype=torch.float16)
    base = dx.AlternateCorrBlock(f1, f2, 4, 3)
    assert blk.coarse_first_level is None and blk._volumes is None
    assert blk.volume_dtype is None and base.volume_dtype is None
    with pytest.raises(AttributeError):
        blk.volume_dtype = torch.float16
    for kind in ("iid", "far"):
        c = _flow(B, H, W, kind, 85)
        assert_same(blk(c), base(c), kind)


def test_cap_counts_the_volumes_real_bytes(dx, monkeypatch):
    B, D, H, W, r = 2, 64, 30, 44, 3
    _force_volumes(dx, monkeypatch)
    n = _nat().load().dxr_alt_volume_numel(B, H, W, 4, 1)
    monkeypatch.setattr(dx.AlternateCorrBlock, "COARSE_VOLUME_MAX_BYTES", 3 * n)
    f1, f2 = _class_fmaps(B, D, H, W, torch.float32)
    b16 = dx.AlternateCorrBlock(f1, f2, 4, r, volume_dtype=torch.float16)
    b32 = dx.AlternateCorrBlock(f1, f2, 4, r)
    assert b16.coarse_first_level == 1 and b16._volumes.numel() == n
    assert b16._volumes.numel() * b16._volumes.element_size() == 2 * n
    assert b32.coarse_first_level == 2
    # below the float16 size both drop level 1
    monkeypatch.setattr(dx.AlternateCorrBlock, "COARSE_VOLUME_MAX_BYTES", 2 * n - 1)
    assert dx.AlternateCorrBlock(f1, f2, 4, r, volume_dtype=torch.float16).coarse_first_level == 2


def test_trainable_block(dx, monkeypatch):
    B, D, H, W, r = 2, 64, 30, 44, 3
    _force_volumes(dx, monkeypatch)
    f1, f2 = _class_fmaps(B, D, H, W, torch.float32)
    with pytest.raises(NotImplementedError, match="float16 coarse volumes"):
        dx.TrainableAlternateCorrBlock(f1.clone().requires_grad_(True), f2, 4, r,
                                       volume_dtype=torch.float16)
    with pytest.raises(NotImplementedError, match="float16 coarse volumes"):
        dx.TrainableAlternateCorrBlock(f1, f2.clone().requires_grad_(True), 4, r,
                                       volume_dtype=torch.float16)
    # float32 volumes train as before; without grad: the base block
    g = dx.TrainableAlternateCorrBlock(f1.clone().requires_grad_(True), f2, 4, r)
    assert g.volume_dtype == torch.float32
    with torch.no_grad():
        ng = dx.TrainableAlternateCorrBlock(f1.clone().requires_grad_(True), f2, 4, r,
                                            volume_dtype=torch.float16)
    assert ng.volume_dtype == torch.float16
    t = _check_block(dx, f1, f2, 4, r, 1, KINDS[:1], cls=dx.TrainableAlternateCorrBlock)
    c = _flow(B, H, W, "iid", 86)
    base = dx.AlternateCorrBlock(f1, f2, 4, r, volume_dtype=torch.float16)
    assert_same(t(c), base(c), "trainable without grad")
    assert not t(c).requires_grad


def test_graph_capture_of_a_float16_volume_lookup_matches_eager(dx, monkeypatch):
    B, D, H, W, r = 2, 64, 30, 44, 3
    _force_volumes(dx, monkeypatch)
    f1, f2 = _class_fmaps(B, D, H, W, torch.float32)
    c = _flow(B, H, W, "iid", 87)
    state = {}

    def step():
        blk = dx.AlternateCorrBlock(f1, f2, 4, r, volume_dtype=torch.float16)
        assert blk.volume_dtype == torch.float16 and blk.coarse_first_level == 1
        state["out"] = blk(c)

    stream = torch.cuda.Stream(device=DEV)
    with torch.no_grad(), torch.cuda.stream(stream):
        step()
        stream.synchronize()
        ref = state["out"].clone()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            step()
        state["out"].zero_()
        g.replay()
        stream.synchronize()
        assert_same(state["out"], ref, "replay")
        assert bool(ref.abs().max() > 0)
