"""GPU: the alternate block's lookups with 16-bit and / or channels-last outputs
(DXR_OUT_F16 / DXR_OUT_BF16 / DXR_OUT_NHWC on ``radius``;
``AlternateCorrBlock(..., out_dtype=, memory_format=)``).

Every check is bit equality against the unflagged call of the same entry point
on the same inputs, converted by torch: ``ref.to(dtype)`` and the channels-last
permutation of ``ref``.  No tolerance is involved; the unflagged call itself is
checked against float64 in tests/test_gpu_alt_oracle.py, whose shapes, operands
and coordinate sets are reused here.  Every bit is compared, those of NaNs (sign
and payload) included: the flagged kernels issue the float32 kernels' arithmetic
instruction by instruction (csrc/out_store.h, "Pinned float32 arithmetic").

Both calls write into a buffer pre-filled with a finite sentinel (1.5: exact in
float16 and bfloat16) with a guard region behind it, so the comparison of whole
buffers also shows that a flagged call writes exactly the elements the unflagged
one writes: the guard keeps its bytes, and the channels of levels a partial call
leaves out keep the sentinel in every pixel's run.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest
import torch

import datagen as dg
from test_gpu_alt_oracle import GUARD, SENTINEL, SHAPES, _seed, _t, coord_set, operands

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F16, BF16, NHWC = 0x100, 0x200, 0x1000
FLAG_SETS = (F16, BF16, NHWC, NHWC | F16, NHWC | BF16)
FORMS = ("mfma_tile", "mfma_ordered", "mfma_ordered_levels2")
POINTS = [("base", 48, r) for r in (0, 3, 4, 6)] + [("tpb2", 80, 4)]
RUNS = [(f, sh, D, r, s) for sh, D, r in POINTS for s in ("uniform", "smooth") for f in FORMS]
RUNS += [(f, "base", 48, 4, "nonfinite") for f in FORMS]
# the remaining radii once each: the compiler fuses the combination's products and sums per
# instantiation (csrc/out_store.h, "Pinned float32 arithmetic"), so every radius is held to the bits
RUNS += [(f, "base", 48, r, "uniform") for r in (1, 2, 5) for f in FORMS[:2]]


@pytest.fixture(scope="module")
def dx():
    import dexiraft_amd
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    dexiraft_amd.load_native()
    return dexiraft_amd


def _nat():
    from dexiraft_amd import _native
    return _native


def _dtype(hi: int) -> torch.dtype:
    return torch.float16 if hi & F16 else torch.bfloat16 if hi & BF16 else torch.float32


def _guarded(n: int, dtype: torch.dtype, off: int = 0) -> torch.Tensor:
    """n + GUARD sentinel elements, starting `off` elements into an allocation."""
    return torch.full((off + n + GUARD,), SENTINEL, dtype=dtype, device=DEV)[off:]


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def assert_same_bits(got: torch.Tensor, want: torch.Tensor, tag: str) -> None:
    """Equal dtype, shape and bits — all of them, a NaN's sign and payload too."""
    assert got.dtype == want.dtype and got.shape == want.shape, tag
    bg, bw = _bits(got), _bits(want)
    same = bg == bw
    if not bool(same.all()):
        i = int((~same).flatten().nonzero()[0])
        raise AssertionError(f"{tag}: {int((~same).sum())} of {same.numel()} elements differ, first "
                             f"at flat index {i}: got {got.flatten()[i].item()!r} want "
                             f"{want.flatten()[i].item()!r}")


def converted(ref: torch.Tensor, hi: int) -> torch.Tensor:
    """What the flags ask for, made by torch from the unflagged float32 NCHW
    result [B, K, H, W]: the flat memory the flagged call must have written."""
    out = ref.to(_dtype(hi))
    if hi & NHWC:
        out = out.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)
    return out.contiguous().flatten()


def check_buffer(buf: torch.Tensor, ref_buf: torch.Tensor, shape, hi: int, tag: str) -> None:
    """The flagged call's guarded buffer against the unflagged call's."""
    torch.cuda.synchronize()
    n = int(np.prod(shape))
    guard = torch.full((GUARD,), SENTINEL, dtype=buf.dtype, device=DEV)
    assert torch.equal(_bits(buf[n:]), _bits(guard)), f"{tag}: the guard behind the output was written"
    assert_same_bits(buf[:n], converted(ref_buf[:n].view(shape), hi), tag)


def _call(form: str, ab, ct, buf, shape: str, D: int, r_flags: int, n_levels: int = 2):
    nat = _nat()
    lib = nat.load()
    B, H, W, L = SHAPES[shape]
    args = (ab._f1_nhwc.data_ptr(), ab._f2_ptrs, ct.data_ptr(), buf.data_ptr(), B, H, W, D, L)
    div = float(np.sqrt(np.float32(D), dtype=np.float32))
    s = nat.stream_of(buf)
    if form == "mfma_tile":
        return lib.dxr_alt_corr_lookup(*args, r_flags, div, s)
    nl = L if form == "mfma_ordered" else n_levels
    n = lib.dxr_alt_workspace_bytes(B, H, W, nl)
    ws = torch.empty(n, dtype=torch.uint8, device=DEV)
    assert n > 0 and ws.data_ptr() % 16 == 0
    if form == "mfma_ordered":
        return lib.dxr_alt_corr_lookup_ws(*args, r_flags, div, ws.data_ptr(), n, s)
    return lib.dxr_alt_corr_lookup_levels_ws(*args, nl, r_flags, div, ws.data_ptr(), n, s)


@lru_cache(maxsize=4)
def coords_of(shape: str, D: int, r: int, cset: str) -> torch.Tensor:
    B, H, W, _ = SHAPES[shape]
    return _t(coord_set(_seed(shape, D, r, cset), cset, B, H, W))


@lru_cache(maxsize=4)
def unflagged(form: str, shape: str, D: int, r: int, cset: str) -> torch.Tensor:
    """The unflagged call's guarded float32 buffer (shared by the flag sets)."""
    B, H, W, L = SHAPES[shape]
    K = L * (2 * r + 1) ** 2
    buf = _guarded(B * K * H * W, torch.float32)
    assert _call(form, operands(shape, D), coords_of(shape, D, r, cset), buf, shape, D, r) == 0
    torch.cuda.synchronize()
    return buf


# --------------------------------------------------------------------------- C-ABI, MFMA forms
@pytest.mark.parametrize("form,shape,D,r,cset", RUNS,
                         ids=[f"{f}-{sh}-D{D}-r{r}-{s}" for f, sh, D, r, s in RUNS])
def test_flagged_mfma_forms_equal_the_unflagged_call_converted(dx, form, shape, D, r, cset):
    B, H, W, L = SHAPES[shape]
    K = L * (2 * r + 1) ** 2
    ref = unflagged(form, shape, D, r, cset)
    if cset == "nonfinite":
        assert torch.isnan(ref[:B * K * H * W]).any()
    if form == "mfma_ordered_levels2":   # levels 2-3 are another call's: sentinel in the reference
        k = (2 * r + 1) ** 2
        assert (ref[:B * K * H * W].view(B, K, H, W)[:, 2 * k:] == SENTINEL).all()
    ab, ct = operands(shape, D), coords_of(shape, D, r, cset)
    for hi in FLAG_SETS:
        buf = _guarded(B * K * H * W, _dtype(hi))
        st = _call(form, ab, ct, buf, shape, D, r | hi)
        assert st == 0, f"{form} flags {hi:#x}: status {st}"
        check_buffer(buf, ref, (B, K, H, W), hi, f"{form} {shape} D={D} r={r} {cset} flags {hi:#x}")


# --------------------------------------------------------------------------- odd C, odd run offsets
@pytest.mark.parametrize("form", FORMS[:2])
@pytest.mark.parametrize("levels,r", [(1, 1), (3, 2)], ids=["C9", "C75"])
def test_odd_channel_counts_and_odd_run_offsets(dx, form, levels, r):
    """C = 9 (one level, r = 1) and C = 75 (three levels of 25: level 1 starts at
    an odd channel): a pixel's run and a level's run start 2-byte aligned only, on
    an even base and on a base one element into the allocation."""
    nat = _nat()
    lib = nat.load()
    B, H, W, D = 2, 18, 21, 48
    f1 = _t(dg.fmap(_seed("odd", levels, 1), B, D, H, W))
    f2 = _t(dg.fmap(_seed("odd", levels, 2), B, D, H, W))
    ab = dx.AlternateCorrBlock(f1, f2, num_levels=levels, radius=r)
    assert ab.coarse_first_level is None
    ct = _t(coord_set(_seed("odd", levels, r), "uniform", B, H, W))
    K = levels * (2 * r + 1) ** 2
    assert K % 2 == 1
    n = B * K * H * W
    div = float(np.sqrt(np.float32(D), dtype=np.float32))

    def call(buf, r_flags):
        args = (ab._f1_nhwc.data_ptr(), ab._f2_ptrs, ct.data_ptr(), buf.data_ptr(), B, H, W, D,
                levels)
        if form == "mfma_tile":
            return lib.dxr_alt_corr_lookup(*args, r_flags, div, nat.stream_of(buf))
        nb = lib.dxr_alt_workspace_bytes(B, H, W, levels)
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
        return lib.dxr_alt_corr_lookup_ws(*args, r_flags, div, ws.data_ptr(), nb, nat.stream_of(buf))

    ref = _guarded(n, torch.float32)
    assert call(ref, r) == 0
    for hi in (F16, BF16, NHWC | F16, NHWC | BF16):
        for off in (0, 1):
            buf = _guarded(n, _dtype(hi), off)
            assert buf.data_ptr() % 4 == 2 * off
            assert call(buf, r | hi) == 0
            check_buffer(buf, ref, (B, K, H, W), hi, f"{form} C={K} flags {hi:#x} base +{off}")


# --------------------------------------------------------------------------- the volume lookup
@lru_cache(maxsize=1)
def volume_case():
    """base, D = 48: the operands, and the volumes of levels 1.. and 2.. ."""
    nat = _nat()
    lib = nat.load()
    B, H, W, L = SHAPES["base"]
    ab = operands("base", 48)
    vols = {}
    for first in (1, 2):
        nv = lib.dxr_alt_volume_numel(B, H, W, L, first)
        vol = torch.full((nv,), float("nan"), device=DEV)
        assert lib.dxr_alt_coarse_volumes(ab._f1_nhwc.data_ptr(), ab._f2_ptrs, B, H, W, 48, L, first,
                                          vol.data_ptr(), nat.stream_of(vol)) == 0
        vols[first] = vol
    return ab, vols


@pytest.mark.parametrize("first", [1, 2])
@pytest.mark.parametrize("r", [3, 4, 5, 8])
def test_volume_lookup_and_the_product_pair(dx, first, r):
    """dxr_alt_volume_lookup from first_level with every flag set: alone (the
    levels below first_level keep the sentinel) and, where the on-the-fly form
    has the radius, after the flagged _levels_ws call into the same tensor — the
    product path — against the same pair unflagged, converted."""
    nat = _nat()
    lib = nat.load()
    shape, D = "base", 48
    B, H, W, L = SHAPES[shape]
    ab, vols = volume_case()
    vol = vols[first]
    K = L * (2 * r + 1) ** 2
    k = (2 * r + 1) ** 2
    n = B * K * H * W
    div = float(np.sqrt(np.float32(D), dtype=np.float32))
    for cset in ("uniform", "nonfinite"):
        ct = coords_of(shape, D, r, cset)

        def run(hi, pair):
            buf = _guarded(n, _dtype(hi))
            if pair:
                assert _call("mfma_ordered_levels2", ab, ct, buf, shape, D, r | hi, first) == 0
            assert lib.dxr_alt_volume_lookup(vol.data_ptr(), ct.data_ptr(), buf.data_ptr(), B, H, W,
                                             L, first, r | hi, div, nat.stream_of(buf)) == 0
            return buf

        for pair in ((False, True) if r <= 6 else (False,)):
            ref = run(0, pair)
            torch.cuda.synchronize()
            low = ref[:n].view(B, K, H, W)[:, :first * k]
            assert bool((low == SENTINEL).all()) != pair      # written by the on-the-fly call only
            assert not (ref[:n].view(B, K, H, W)[:, first * k:] == SENTINEL).all()
            for hi in FLAG_SETS:
                check_buffer(run(hi, pair), ref, (B, K, H, W), hi,
                             f"volume first={first} r={r} {cset} pair={pair} flags {hi:#x}")


# --------------------------------------------------------------------------- overflow and NaN
def test_float16_overflow_and_nan(dx):
    """fmaps scaled so that outputs pass 65504, and a NaN coordinate: +-inf and
    NaN exactly where .half() of the float32 result has them."""
    nat = _nat()
    lib = nat.load()
    B, H, W, D, L, r = 2, 18, 21, 48, 4, 3
    f1 = _t(dg.fmap(_seed("ovf", 1), B, D, H, W)) * 300.0
    f2 = _t(dg.fmap(_seed("ovf", 2), B, D, H, W)) * 300.0
    ab = dx.AlternateCorrBlock(f1, f2, num_levels=L, radius=r)
    c = coord_set(_seed("ovf", 3), "uniform", B, H, W)
    c[0, 0, 3, 5] = np.nan
    c[1, :, 4, 6] = np.nan          # both fractions NaN: every product has two NaN operands
    c[1, 0, 9, 9], c[1, 1, 9, 9] = np.inf, np.nan
    ct = _t(c)
    K = L * (2 * r + 1) ** 2
    n = B * K * H * W
    div = float(np.sqrt(np.float32(D), dtype=np.float32))

    def call(buf, r_flags):
        return lib.dxr_alt_corr_lookup(ab._f1_nhwc.data_ptr(), ab._f2_ptrs, ct.data_ptr(),
                                       buf.data_ptr(), B, H, W, D, L, r_flags, div,
                                       nat.stream_of(buf))

    ref = _guarded(n, torch.float32)
    assert call(ref, r) == 0
    torch.cuda.synchronize()
    r32 = ref[:n]
    assert torch.isfinite(r32[~torch.isnan(r32)]).all()
    assert (r32 > 65520).any() and (r32 < -65520).any() and torch.isnan(r32).any()
    for hi in (F16, NHWC | F16):
        buf = _guarded(n, torch.float16)
        assert call(buf, r | hi) == 0
        check_buffer(buf, ref, (B, K, H, W), hi, f"overflow flags {hi:#x}")
        want = converted(r32.view(B, K, H, W), hi)
        got = buf[:n]
        assert torch.equal(torch.isposinf(got), torch.isposinf(want)) and torch.isposinf(got).any()
        assert torch.equal(torch.isneginf(got), torch.isneginf(want)) and torch.isneginf(got).any()
        assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.isnan(got).any()


# --------------------------------------------------------------------------- Python
KINDS = [(dt, mf) for dt in (None, torch.float32, torch.float16, torch.bfloat16)
         for mf in (None, torch.contiguous_format, torch.channels_last)]


def _python_case(dx, D, monkeypatch, volumes):
    B, H, W = 2, 18, 21
    if volumes:
        monkeypatch.setattr(dx.AlternateCorrBlock, "COARSE_MIN_QUERIES", 0)
    f1 = _t(dg.fmap(_seed("py", D, 1), B, D, H, W))
    f2 = _t(dg.fmap(_seed("py", D, 2), B, D, H, W))
    cs = [_t(coord_set(_seed("py", D, s), s, B, H, W)) for s in ("uniform", "nonfinite")]
    base = dx.AlternateCorrBlock(f1, f2, num_levels=4, radius=4)
    assert (base.coarse_first_level is not None) == volumes
    for c in cs:
        ref = base(c)
        assert ref.dtype == torch.float32 and ref.is_contiguous()
        assert tuple(ref.shape) == (B, 4 * 81, H, W)
        for dt, mf in KINDS:
            ab = dx.AlternateCorrBlock(f1, f2, num_levels=4, radius=4, out_dtype=dt, memory_format=mf)
            assert (ab.coarse_first_level is not None) == volumes
            got = ab(c)
            want_dt = dt or torch.float32
            tag = f"D={D} volumes={volumes} {dt} {mf}"
            assert got.dtype == want_dt and got.shape == ref.shape, tag
            want = ref.to(want_dt)
            if mf is torch.channels_last:
                assert got.is_contiguous(memory_format=torch.channels_last), tag
                assert got.stride() == (H * W * 324, 1, W * 324, 324), tag
                want = want.contiguous(memory_format=torch.channels_last)
                assert_same_bits(got.permute(0, 2, 3, 1), want.permute(0, 2, 3, 1), tag)
            else:
                assert got.is_contiguous(), tag
                assert_same_bits(got, want, tag)
            with pytest.raises(TypeError):
                ab(c, out_dtype=torch.float16)
            with pytest.raises(TypeError):
                ab(c, memory_format=torch.channels_last)


def test_python_block_on_the_fly(dx, monkeypatch):
    _python_case(dx, 48, monkeypatch, volumes=False)


def test_python_block_with_coarse_volumes(dx, monkeypatch):
    _python_case(dx, 48, monkeypatch, volumes=True)


def test_python_block_valu_form_falls_back_to_the_same_bits(dx, monkeypatch):
    """D = 36: the VALU form declines the flags and the block converts the
    float32 NCHW call — the same converted bits as the native forms give."""
    nat = _nat()
    lib = nat.load()
    P = 1 << 12
    ptrs = (nat.ctypes.c_void_p * 4)(P, P, P, P)
    assert lib.dxr_alt_corr_lookup(P, ptrs, P, P, 1, 16, 16, 36, 4, 4 | F16, 6.0, None) == \
        nat.DXR_EUNSUPPORTED
    _python_case(dx, 36, monkeypatch, volumes=False)
