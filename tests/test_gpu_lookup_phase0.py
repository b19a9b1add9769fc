"""Phase 0 of the product lookup, bit for bit against the numpy oracle.

The lookup's coordinate round trip divides by a workgroup-uniform divisor with a
short division where that is proven exact (divisors 1 ... 511 and finite
coordinates, scripts/check_uniform_div.cpp) and with the full IEEE division
elsewhere: a level of size 1 (divisor 0), non-finite coordinates.  These cases
drive every branch of that choice, in both workgroup shapes:

  * maps 9 x 20 (levels 9x20, 4x10, 2x5, 1x2: level 3 has height 1, divisor 0),
    8 x 16 (level 3 is 1x2 too, N % 32 == 0) and 7 x 11 with two levels
    (N = 77: N % 16 != 0 and N % 32 != 0);
  * float32 and bfloat16 pyramids; radii 1, 3 and 4;
  * the one-round grid (256 x 16 workgroups: few pairs) and the multi-round
    grid (512 x 32: enough pairs that ceil(N / 32) * levels * B > 1024, the rule
    test_lookup_grid_shapes_agree_on_padded_pyramid uses);
  * coordinate kinds, one per pair of the batch in turn: normal jitter, exact
    integers, exact half-integers, +-0, one ulp either side of an integer (samples
    within an ulp of a cell boundary), off the map by more than the window,
    and +-1e7 / +-3e38 / +-inf / NaN, sparse (one lane of a wave) and dense.

The reference is oracle.corr_lookup on the block's own pyramid (widened to
float32, as the kernel reads it): equal bits wherever it is a number, NaN exactly
where it is NaN.  The CPU test checks first that the oracle and tests/torch_ref.py
agree on a height-1 level, where the reference divides by zero.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest
import torch

import datagen as dg
import oracle
from torch_ref import TorchCorrBlock

DEV = "cuda:0"
D = 64
MAPS = {"9x20": (9, 20, 4), "8x16": (8, 16, 4), "7x11": (7, 11, 2)}   # H, W, levels
KINDS = ["normal", "integer", "half", "zero", "ulp_up", "ulp_down", "off_map", "special_sparse",
         "special_dense"]
SPECIALS = np.array([1e7, -1e7, 3e38, -3e38, np.inf, -np.inf, np.nan], dtype=np.float32)


def coords_of_kind(kind: str, seed: int, H: int, W: int) -> np.ndarray:
    """[2, H, W] float32."""
    integer = dg.coords(seed, 1, H, W, "integer", 3.0)[0]
    if kind == "normal":
        return dg.coords(seed, 1, H, W, "normal", 2.0)[0]
    if kind == "integer":
        return integer
    if kind == "half":
        return integer + np.float32(0.5)
    if kind == "zero":   # +0 and -0 in a checkerboard, opposite signs on the two axes
        sign = np.where((np.arange(H)[:, None] + np.arange(W)[None, :]) % 2 == 0, 1.0, -1.0)
        return np.stack([np.copysign(0.0, sign), np.copysign(0.0, -sign)]).astype(np.float32)
    if kind == "ulp_up":
        return np.nextafter(integer, np.float32(np.inf))
    if kind == "ulp_down":
        return np.nextafter(integer, np.float32(-np.inf))
    if kind == "off_map":   # further than the window (r + 2 cells at level 0) on either side
        side = np.where(np.arange(W)[None, :] % 2 == 0, 1.0, -1.0)
        return (integer + np.float32(40.0) * side).astype(np.float32)
    c = dg.coords(seed, 1, H, W, "normal", 2.0)[0].copy()
    flat = c.reshape(2, H * W)
    if kind == "special_sparse":   # one query in 23: most waves hold one such lane, some none
        idx = np.arange(5, H * W, 23)
        flat[0, idx] = SPECIALS[np.arange(len(idx)) % len(SPECIALS)]
        flat[1, idx[::2]] = SPECIALS[(np.arange(len(idx[::2])) + 3) % len(SPECIALS)]
        return c
    assert kind == "special_dense"
    flat[0] = SPECIALS[np.arange(H * W) % len(SPECIALS)]
    flat[1, 1::2] = SPECIALS[(np.arange(H * W)[1::2] // 2 + 2) % len(SPECIALS)]
    return c


def batch_coords(name: str, B: int) -> np.ndarray:
    """Pair b holds kind b % len(KINDS), with its own seed."""
    H, W, _ = MAPS[name]
    return np.stack([coords_of_kind(KINDS[b % len(KINDS)], 900 + b, H, W) for b in range(B)])


def batch_size(name: str, shape: str) -> int:
    H, W, L = MAPS[name]
    per_pair = -(-(H * W) // 32) * L          # 32-query workgroups per pair
    if shape == "one_round":
        B = len(KINDS)
        assert per_pair * B <= 1024
        return B
    return 1024 // per_pair + 1                # the first batch past one dispatch round


def test_oracle_agrees_with_torch_on_a_height_one_level():
    """9 x 20 with 4 levels: level 3 is 1 x 2, its y divisor 0.  The oracle's
    lookup and F.grid_sample (CPU) on the same float32 pyramid: the same NaNs and
    the same numbers elsewhere, for finite coordinates of every kind."""
    H, W, L = MAPS["9x20"]
    f1, f2 = dg.fmap(11, 1, D, H, W), dg.fmap(12, 1, D, H, W)
    tb = TorchCorrBlock(torch.from_numpy(f1), torch.from_numpy(f2), num_levels=L, radius=3)
    assert tuple(tb.levels[3].shape[-2:]) == (1, 2)
    pyr = [lv[:, 0].numpy() for lv in tb.levels]
    for kind in ["normal", "integer", "half", "zero", "ulp_up", "off_map"]:
        c = coords_of_kind(kind, 77, H, W)[None]
        with np.errstate(all="ignore"):
            ref = oracle.corr_lookup(pyr, c, 3)
        got = tb(torch.from_numpy(c)).numpy()
        assert np.array_equal(np.isnan(got), np.isnan(ref)), kind
        assert np.isnan(ref[:, 3 * 49:]).any(), "the height-1 level makes NaNs"
        ok = ~np.isnan(ref)
        assert np.array_equal(got[ok], ref[ok]), kind


@pytest.fixture(scope="module")
def dx():
    import dexiraft_amd
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    dexiraft_amd.load_native()
    return dexiraft_amd


@lru_cache(maxsize=None)
def fmaps(name: str, dtype: str, B: int):
    H, W, _ = MAPS[name]
    td = torch.float32 if dtype == "f32" else torch.bfloat16
    f1 = torch.from_numpy(dg.fmap(21, B, D, H, W, "fnet")).to(DEV).to(td)
    f2 = torch.from_numpy(dg.fmap(22, B, D, H, W, "fnet")).to(DEV).to(td)
    return f1, f2


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["one_round", "multi_round"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(MAPS))
def test_lookup_bits_equal_the_oracle(dx, name, dtype, shape):
    H, W, L = MAPS[name]
    B = batch_size(name, shape)
    f1, f2 = fmaps(name, dtype, B)
    c = batch_coords(name, B)
    ct = torch.from_numpy(c).to(DEV)
    pyr = None
    for r in (1, 3, 4):
        cb = dx.CorrBlock(f1, f2, num_levels=L, radius=r)
        if pyr is None:   # the pyramid does not depend on the radius
            pyr = [cb.corr_pyramid[lvl][:, 0].cpu().numpy() for lvl in range(L)]
        got = cb(ct).cpu().numpy()
        with np.errstate(all="ignore"):
            ref = oracle.corr_lookup(pyr, c, r)
        assert got.shape == ref.shape
        nan = np.isnan(ref)
        assert np.array_equal(np.isnan(got), nan), (r, int((np.isnan(got) != nan).sum()))
        assert np.array_equal(got[~nan].view(np.uint32), ref[~nan].view(np.uint32)), \
            (r, int((got[~nan].view(np.uint32) != ref[~nan].view(np.uint32)).sum()))
        for k, kind in enumerate(KINDS):   # the kinds do what they are for
            if kind.startswith("special"):
                assert np.isnan(got[k]).any(), kind
            elif kind == "off_map" and (H, W) != (9, 20) and (H, W) != (8, 16):
                assert not got[k].any(), kind   # (a height-1 level answers NaN instead)
