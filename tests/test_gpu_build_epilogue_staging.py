"""The build epilogue's level-0 staging (csrc/corr_build.hip paged_epilogue) at
the smallest shapes where it can go wrong.

A wave stages its 32 queries' level-0 rows through LDS in two rounds and
streams each round out as 1 KiB stores; which rows a round holds, which lanes
read which query back, and where the rows land in the page are all index
arithmetic that a slip breaks silently for some rows of some queries only.
Every case therefore compares the WHOLE built pyramid, through the unpack entry
point (``CorrBlock.corr_pyramid``), with the float64 oracle's:

  ragged    fmap 9 x 17, D = 32, B = 1: two tile rows and two tile columns, both
            ragged; N = 153 = one full 128-query page + a 25-query one (lanes
            past N, a half unit);
  one_tile  fmap 8 x 16, D = 16, B = 2: exactly one tile and one partial page;
  levels    fmap 24 x 40, D = 64, B = 1 with num_levels 1, 2, 3 and 4: the early
            returns after level 0 and level 1 sit between the staging barriers;

each for f32 fmaps into an f32 pyramid, f32 fmaps into a float16 pyramid and
bf16 fmaps (the 2-byte store branch is its own code).  Tolerances are the
existing accuracy tests' for each cell type, not new ones:

  f32       test_gpu_parity.test_split_build_f32_accuracy: RTOL of max|ref|;
  float16   test_gpu_pyr16.test_pyr16_accuracy_against_float64: half a float16
            ulp of ref + RTOL max|ref|;
  bf16      test_gpu_parity.test_bf16_mode_within_its_tolerance (its float64
            comparison, on the same bf16-rounded inputs): 2^-8 |ref| + 1e-5 max|ref|.

``test_oracle_alone_is_within_the_tolerances`` (no GPU) checks that float32
arithmetic by the oracle itself, rounded to the cell type, meets those bounds
on these inputs, so a failure of a GPU case is the kernel's.  f32 NCHW and NHWC
fmaps must give the same pages bit for bit, and a non-finite operand pixel
(whose pages the wave writes twice through the same epilogue) must give the
exact-f32 build's pyramid, as test_prescaled_build_nonfinite_fallback_forms asks.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import datagen as dg
import oracle
from conftest import tolerance_check
from test_gpu_parity import RTOL, _build_exact_f32
from test_gpu_pyr16 import F16_MIN_NORMAL
from test_gpu_pyr16 import RTOL as PYR16_RTOL

DEV = "cuda:0"
CASES = {"ragged": (1, 32, 9, 17), "one_tile": (2, 16, 8, 16), "levels": (1, 64, 24, 40)}
SEEDS = {"ragged": 2310, "one_tile": 2320, "levels": 2330}
BUILDS = [("ragged", 4), ("one_tile", 4), ("levels", 1), ("levels", 2), ("levels", 3), ("levels", 4)]
FORMS = ["f32", "pyr16", "bf16"]


@pytest.fixture(scope="module")
def dx():
    import dexiraft_amd
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    dexiraft_amd.load_native()
    return dexiraft_amd


@functools.lru_cache(maxsize=None)
def _fmaps(case: str, bf16: bool):
    """Host fmaps of a case (fnet-like: large, positively biased cells); bf16:
    rounded to bfloat16 (RNE, as .bfloat16() on the device) and widened again."""
    B, D, H, W = CASES[case]
    f1 = dg.fmap(SEEDS[case], B, D, H, W, "fnet")
    f2 = dg.fmap(SEEDS[case] + 1, B, D, H, W, "fnet")
    if bf16:
        f1 = torch.from_numpy(f1).bfloat16().float().numpy()
        f2 = torch.from_numpy(f2).bfloat16().float().numpy()
    return f1, f2


@functools.lru_cache(maxsize=None)
def _ref64(case: str, bf16: bool):
    """The float64 oracle's four levels, computed once per case and shared
    (num_levels L is its first L levels).  Read-only."""
    pyr = oracle.corr_pyramid(*_fmaps(case, bf16), 4, np.float64)
    for lev in pyr:
        lev.setflags(write=False)
    return pyr


def _check_level(got: np.ndarray, ref: np.ndarray, form: str, what: str) -> None:
    """One level against the float64 oracle under the bound of its cell type
    (module docstring); prints the figures before it asserts."""
    a = np.abs(ref)
    err = np.abs(got.astype(np.float64) - ref)
    if form == "f32":
        print(f"{what}: max err {err.max():.3e}, bound {RTOL * a.max():.3e}")
        tolerance_check(got, ref, RTOL)
        return
    if form == "pyr16":
        half_ulp = np.where(a < F16_MIN_NORMAL, 2.0 ** -25, a * 2.0 ** -11)
        bound = half_ulp + PYR16_RTOL * a.max()
    else:
        bound = 2.0 ** -8 * a + 1e-5 * a.max()
    print(f"{what}: max err {err.max():.3e}, max err/bound {(err / bound).max():.3f}, "
          f"max|ref| {a.max():.3e}")
    assert np.isfinite(got).all(), what
    bad = np.argwhere(err > bound)
    assert bad.size == 0, f"{what}: {len(bad)} cells out of bound, first (query, row, col) {bad[0]}"


def _block(dx, case: str, form: str, levels: int, nhwc: bool = False):
    f1, f2 = (torch.from_numpy(f).to(DEV) for f in _fmaps(case, form == "bf16"))
    if form == "bf16":
        f1, f2 = f1.bfloat16(), f2.bfloat16()
    if nhwc:
        f1 = f1.contiguous(memory_format=torch.channels_last)
        f2 = f2.contiguous(memory_format=torch.channels_last)
    kw = {"pyramid_dtype": torch.float16} if form == "pyr16" else {}
    return dx.CorrBlock(f1, f2, num_levels=levels, **kw)


def test_oracle_alone_is_within_the_tolerances():
    """float32 arithmetic by the oracle, rounded once to the cell type, against
    its own float64 result: inside every bound the GPU cases use, on their inputs."""
    for case in CASES:
        for form in FORMS:
            bf = form == "bf16"
            ref = _ref64(case, bf)
            p32 = oracle.corr_pyramid(*_fmaps(case, bf), 4, np.float32)
            for lvl in range(4):
                t = torch.from_numpy(np.ascontiguousarray(p32[lvl], dtype=np.float32))
                if form == "pyr16":
                    t = t.half().float()
                elif bf:
                    t = t.bfloat16().float()
                _check_level(t.numpy(), ref[lvl], form, f"oracle f32 {case} {form} level {lvl}")


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case,levels", BUILDS)
def test_built_pyramid_matches_float64_oracle(dx, case, levels, form):
    B, D, H, W = CASES[case]
    cb = _block(dx, case, form, levels)
    assert cb._buf.dtype == {"f32": torch.float32, "pyr16": torch.float16,
                             "bf16": torch.bfloat16}[form]
    ref = _ref64(case, form == "bf16")
    pyr = cb.corr_pyramid
    assert len(pyr) == levels
    for lvl in range(levels):
        got = pyr[lvl][:, 0].cpu().numpy()
        assert got.shape == ref[lvl].shape == (B * H * W, H >> lvl, W >> lvl)
        _check_level(got, ref[lvl], form, f"{case} L={levels} {form} level {lvl}")


@pytest.mark.gpu
@pytest.mark.parametrize("case,levels", BUILDS)
def test_f32_nchw_and_nhwc_fmaps_give_identical_pages(dx, case, levels):
    a = _block(dx, case, "f32", levels)
    b = _block(dx, case, "f32", levels, nhwc=True)
    assert torch.equal(a._buf, b._buf)


@pytest.mark.gpu
def test_nonfinite_pixels_rewritten_through_the_same_epilogue(dx):
    """One inf channel in one query pixel and one in one target pixel (ragged
    case, f32): the waves that see them write their pages, recompute them on
    the exact-f32 MFMA and write them again through the same epilogue.  Against
    the exact-f32 build: NaN and inf patterns (signs too) equal, f32 class
    everywhere else, at every level."""
    B, D, H, W = CASES["ragged"]
    f1, f2 = (torch.from_numpy(f).to(DEV).clone() for f in _fmaps("ragged", False))
    f1[0, 5, 2, 7] = float("inf")                # query (2, 7): +-inf row
    f2[0, 9, 8, 16] = float("inf")               # target (8, 16), the ragged corner tile
    base = _build_exact_f32(f1, f2)
    cb = dx.CorrBlock(f1, f2)
    for lvl in range(4):
        got, ref = cb.corr_pyramid[lvl][:, 0], base[lvl]
        assert torch.equal(torch.isnan(got), torch.isnan(ref)), lvl
        assert torch.equal(torch.isinf(got), torch.isinf(ref)), lvl
        assert torch.equal(got[torch.isinf(ref)], ref[torch.isinf(ref)]), lvl
        fin = torch.isfinite(ref)
        assert fin.any() and not fin.all(), lvl
        err = (got[fin] - ref[fin]).abs().max().item()
        print(f"level {lvl}: finite cells {int(fin.sum())}, max err {err:.3e}, "
              f"max|ref| {ref[fin].abs().max().item():.3e}")
        assert err <= 1e-5 * ref[fin].abs().max().item(), lvl
