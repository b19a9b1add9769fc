"""float64 oracle, per-cell bounds and host emulation of the forward pyramid
build (``dxr_corr_pyramid_build`` / ``_build_ws``, csrc/corr_build.hip, planned by
csrc/build_plan.h).  numpy, ``datagen`` and ``oracle.corr_oracle`` only: no code
under test.

The operation.  Level 0 is C[q, t] = sum_k f1[k, q] f2[k, t] / sqrt(D) (float32
sqrt), level l + 1 the floor-mode 2 x 2 average of level l over the target dims.
Per cell ``reference`` gives the float64 value ``ref`` and

    M    the same pyramid on |f1|, |f2|: sum_k |a_k| |b_k| / sqrt(D), pooled
    A    the pixel maxima max_k |x_k| (Aq of the query, At of the target)
    T    masked sums: Tq[q, t] = sum over k with a_k != 0 of |b_k|, Tt the mirror
         (a zero operand splits into zeros: its products add no error)

u = 2^-24.  The eleven planner paths are four arithmetic families.

``pair_scaled`` -- split_pairs_kernel + corr_build_dma_kernel (f32 fmaps, workspace)
------------------------------------------------------------------------------------
corr_build.hip, "Round 3": (1) every pixel is scaled by 2^s, s = 14 - e for its
max = f 2^e (``pixel_scale``), so |X| = |x 2^s| < 2^14; hi = RNE_f16(X),
lo = RNE_f16(X - hi) (``split16_f16_record``, csrc/mfma_operands.h).  (2) "lo*hi,
hi*lo, hi*hi into ONE f32 accumulator (f16 x f16 products are exact in f32; 3
roundings per 16 k against the exact-f32 MFMA's 8)"; the epilogue "undoes both
pixels' scales (ldexp by -(s_q + s_t), exact)"; then x / sqrt(D), one division
(``scale_acc``) or folded into the ldexp where sqrt(D) is a power of two.

 * Chain: 3 D / 16 MFMA steps on one float32 accumulator, counted as
   tests/test_gpu_gru.py counts: the steps plus the 16 products inside a step,
   each at most u of the sum of magnitudes (<= M); one more for the division:
   (3 D / 16 + 16 + 1) u M.
 * Pair: float16 carries 11 significand bits.  For X in [2^e, 2^(e+1)):
   |X - hi| <= 2^(e-11), the remainder is exact in float32 and is rounded to lo
   with at most 2^(e-23) <= 2^-23 |X| ("represents every element to <= 2^-23
   |x|", Round 3 (1)).  The dropped lo x lo is at most 2^-22 |a b|.  Together
   2 2^-23 + 2^-22 = 2^-21 of M, the allowance tests/test_gpu_alt_train.py gives
   the same split.
 * Tail: where the remainder is below 2^-14 it lands on float16's subnormal
   grid, spacing 2^-24, whatever X: |X - hi - lo| <= 2^-25 in scaled units, in
   x's units 2^-25 2^(e-14) <= 2^-38 A for a pixel maximum A >= 2^(e-1) (Round 3
   (1): "more than 2^16 below its pixel's max (then to <= 2^-39 of that max)",
   2^-39 of 2^e there).  Per product 2^-38 (Aq |b_k| + At |a_k|), summed over the
   k with the other operand non-zero: 2^-38 (Aq Tq + At Tt) / sqrt(D).
 * Below 2^-14 hi is itself on the subnormal grid and the low part is no longer
   2^-11 of the element but up to 2^-25: the dropped lo x lo is then up to
   2^-25 (2^-11 |B| + 2^-25) in scaled units, 2^-11 of the tail above plus
   2^-50 2^-(s_q + s_t) <= 2^-76 Aq At per channel.
 * Unscale: exact unless the result is a float32 subnormal; that and the
   division's subnormal result are allowed 2^-149 in all.

    b0 = ((3 D / 16 + 17) u + 2^-21) M
         + (2^-38 (1 + 2^-11) (Aq Tq + At Tt) + D 2^-76 Aq At) / sqrt(D) + 2^-149

``pair_unscaled`` -- corr_build_split_kernel (f32 fmaps, no workspace)
---------------------------------------------------------------------
mfma_operands.h, "The float16 pair split": hi = RNE_f16(x),
lo = RNE_f16((x - hi) 2^11), no scale: "lo carries the only rounding: <= 2^-22 |x|
while hi is normal, <= 2^-36 absolute below"; tests/test_gpu_parity.py's
test_linearity documents the same floor.  By the argument above the relative
part is 2^-23 |x| here too; lo's grid is 2^-24 2^-11 = 2^-35 in x's units once
(x - hi) 2^11 < 2^-14, so the tail is 2^-36 per operand, independent of the pixel.
Below 2^-14 hi is on the subnormal grid and x - hi is up to 2^-25 whatever x, so
the dropped lo x lo is up to 2^-25 (2^-11 |b| + 2^-25): as much again, and 2^-50
per channel where both are that small: 2^-35 (Tq + Tt) / sqrt(D) + D 2^-50 / sqrt(D).
corr_build_split_kernel's K loop: "hi*hi into acc, the
two cross products into acc2", then ``fmaf(acc2, 2^-11, acc)``, "Combine (one
rounding)": a chain of D / 16 + 16 on M, one of 2 D / 16 + 16 on the cross terms
(<= 2^-10 M), the combination and the division.

    b0 = ((D / 16 + 18) u + (2 D / 16 + 16) u 2^-10 + 2^-21) M
         + (2^-35 (Tq + Tt) + D 2^-50) / sqrt(D) + 2^-149

``exact`` -- corr_build_f32_kernel (v_mfma_f32_32x32x2_f32)
-----------------------------------------------------------
Two products per MFMA, "8 x 64 for v_mfma_f32_32x32x2_f32" per 16 k ("3 roundings
per 16 k against the exact-f32 MFMA's 8"); K is staged in 16s (BK), the remainder
zero-filled: 8 ceil(D / 16) steps, 2 products inside one, the division.  No split.

    b0 = (8 ceil(D / 16) + 3) u M + 2^-149

``rec16`` -- 16-bit operands (pack + DMA16, DMA16 NHWC, bf16 q2, bf16 scalar)
-----------------------------------------------------------------------------
One exact product per element (bf16 x bf16 and f16 x f16 are exact in float32,
corr_build_dma_kernel's comment on OPK = DMA_F16); 32-channel stages of two
16-deep MFMA steps (BKH; a last partial stage is zero-filled): 2 ceil(D / 32)
steps, 16 inside, the division.  The reference is taken on the rounded inputs.

    b0 = (2 ceil(D / 32) + 17) u M + 2^-149

float16 records below 2^-14 (measured, not documented by the kernel: its comment on
OPK = DMA_F16 promises "the f32 matmul of the widened fmaps to accumulation
rounding").  One v_mfma_f32_32x32x16_f16 at a time, on an MI355X: the 16 products
and the accumulator of a step are aligned to the largest exponent among them and
each is cut off 24 bits below it (1 + 15 products of 2^-15 (1 + 2^-10) gives
1.001e04 where the sum is 1.001e078); and a subnormal float16 operand enters with
the exponent 2^-14 of its format, not its own: with 2^-20 x 1 as the largest
product, 2^-19 x 2^-10 (1 + 2^-10) is added as 2^-29, its 2^-39 lost, and a product
of 2^-39 is lost altogether, although the sum is 2^-20 and float32 holds 2^-43
beside it.  The cut lies 24 bits below the largest *nominal* product
n_k = max(|a_k|, 2^-14) max(|b_k|, 2^-14) (over a_k b_k != 0).  With operands in the
normal range n_k = |a_k b_k| and the cut is what the chain count above stands
for, as on every other path.  What a subnormal operand adds is counted: 17
addends per step, each cut below u n_max <= u sum of the step's n_k, less what
the products' own magnitudes already allow:

    b0 += 17 u (Mn - M),   Mn = sum_k n_k / sqrt(D)     (float16 operands only)

bfloat16's subnormals lie below 2^-126 and are outside every case here.

Levels 1..3 (``paged_epilogue``: "Every pooled value is computed from the f32
values of the level above, in the reference's window order ((v00+v01)+v10)+v11
(F.avg_pool2d), then rounded to OT once"): the pooled bound of the level above
plus four roundings of u on the magnitudes pooled (the three additions; the
fourth is the issue's allowance, the factor 1/4 being exact):

    b_(l+1) = pool(b_l) + 4 u (M_(l+1) + pool(b_l))

Cell type: one rounding to nearest even (``to_out``), half a unit in the last
place of the format, taken at |ref| + b since a value within b of a rounding
boundary may round the other way.  For a magnitude in [2^e, 2^(e+1)) that is
2^(e-8) in bfloat16 (8 significand bits: between 2^-9 and 2^-8 of the magnitude)
and max(2^(e-11), 2^-25) in float16 (11 bits; spacing 2^-24 below 2^-14).  A
float16 value of 65520 or more is +-inf (v_cvt_f16_f32): a cell with
|ref| - b >= 65520 must be that inf, one with |ref| + b < 65520 must be finite.
A correct rounding uses this term up to all of it, so for 16-bit cells the half
of the bound that ``emulate`` has to leave is asked of its float32 values
against b; its cells are held to the whole bound.

Exactness: a cell with M == 0 is exactly 0; every other cell is finite (float16
cells: see above).  No constant here comes from a measured error of the kernels.

``emulate`` restates each family on the host so that it meets these contracts
exactly: an MFMA step is the exact sum of its products added to the float32
accumulator with one rounding.  tests/test_build_bound_cpu.py holds it to half
of the bound and each flawed variant (``FLAWS``) to more than the whole.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import datagen as dg
from oracle import corr_oracle as co

F32 = np.float32
U = 2.0 ** -24
PQ, TH, TW = 128, 8, 16                       # page queries, tile rows, tile cols
F16_INF_FROM = 65520.0                        # RNE: the first value that rounds to inf

# name -> (B, H, W) and what it is there for
CASES = {
    "ragged": (1, 9, 20),    # N = 180: a 128-query page + 52; 2 x 2 ragged tiles; floor-mode
                             # remainders of rows (9-4) and of columns (5-2); W % 4 == 0
    "odd": (1, 9, 17),       # scalar staging, the any-W DMA path
    "even": (1, 10, 18),     # float2 target units
    "two": (2, 8, 16),       # one whole tile, a second pair, no remainder anywhere
    "whole": (1, 33, 44),    # 6 x 15 = 90 DMA units: more than an eighth of the 512 dispatch
                             # slots, so dma_grid keeps whole units (the small cases all run as
                             # tail quarter units); 12 query pages, the last partial
}
KINDS = ("uniform", "wide")
FAMILIES = ("pair_scaled", "pair_unscaled", "exact", "rec16")
FLAWS = ("one_cross", "last_stage_cross", "no_lo", "unscaled_split", "pool_of_rounded",
         "pool_ceil", "partial_page_shift")

# kernel names as include/dexiraft_corr.h's "Kernels by request" spells them
DMA_NCHW = "split_pairs_kernel<NCHW> + corr_build_dma_kernel"
DMA_NHWC = "split_pairs_kernel<NHWC> + corr_build_dma_kernel"
SPLIT_F4 = "corr_build_split_kernel<float4>"
SPLIT_F2 = "corr_build_split_kernel<float2>"
SPLIT_NHWC = "corr_build_split_kernel<NHWC>"
EXACT_VEC = "corr_build_f32_kernel<vec>"
EXACT_SCALAR = "corr_build_f32_kernel<scalar>"
PACK_DMA16 = "pack_bf16_kernel + corr_build_dma_kernel"
DMA16_NHWC = "corr_build_dma_kernel"
BF16_Q2 = "corr_build_bf16_q2_kernel"
BF16_ONE = "corr_build_bf16_kernel"

Request = namedtuple("Request", "id operand layout ws algo cells case D family path")


def _requests():
    """Every build request tests/test_gpu_build_per_cell.py sends, with the kernel
    it must reach (by hand from the header's table; tests/test_build_plan.py asks
    the planner) and the arithmetic family of that kernel."""
    t = []

    def add(id_, operand, layout, ws, algo, cells, case, D, family, path):
        t.append(Request(id_, operand, layout, ws, algo, cells, case, D, family, path))

    ps, pu, ex, rc = FAMILIES
    # pre-split f16 pairs + LDS-DMA build: any W, three cell types, both layouts
    add("dma-nchw", "f32", "nchw", True, "auto", "f32", "ragged", 48, ps, DMA_NCHW)
    add("dma-nchw-d256", "f32", "nchw", True, "auto", "f32", "ragged", 256, ps, DMA_NCHW)
    add("dma-nchw-odd", "f32", "nchw", True, "auto", "f32", "odd", 48, ps, DMA_NCHW)
    add("dma-nchw-two", "f32", "nchw", True, "auto", "f32", "two", 48, ps, DMA_NCHW)
    add("dma-nchw-whole", "f32", "nchw", True, "auto", "f32", "whole", 48, ps, DMA_NCHW)
    add("dma-nchw-bf16cells", "f32", "nchw", True, "auto", "bf16", "ragged", 48, ps, DMA_NCHW)
    add("dma-nchw-f16cells", "f32", "nchw", True, "auto", "f16", "ragged", 48, ps, DMA_NCHW)
    add("dma-nhwc", "f32", "nhwc", True, "auto", "f32", "ragged", 48, ps, DMA_NHWC)
    add("dma-nhwc-odd", "f32", "nhwc", True, "auto", "f32", "odd", 48, ps, DMA_NHWC)
    add("dma-nhwc-f16cells", "f32", "nhwc", True, "auto", "f16", "ragged", 48, ps, DMA_NHWC)
    # register split builds (no workspace)
    add("split-f4", "f32", "nchw", False, "auto", "f32", "ragged", 48, pu, SPLIT_F4)
    add("split-f4-two", "f32", "nchw", False, "auto", "f32", "two", 48, pu, SPLIT_F4)
    add("split-f4-bf16cells", "f32", "nchw", False, "auto", "bf16", "ragged", 48, pu, SPLIT_F4)
    add("split-f2", "f32", "nchw", False, "auto", "f32", "even", 48, pu, SPLIT_F2)
    add("split-nhwc", "f32", "nhwc", False, "auto", "f32", "ragged", 48, pu, SPLIT_NHWC)
    add("split-nhwc-even", "f32", "nhwc", False, "auto", "f32", "even", 48, pu, SPLIT_NHWC)
    # exact-f32 MFMA build: by request, and as the fallback of D % 16 != 0 and odd W
    add("exact-vec", "f32", "nchw", False, "exact", "f32", "ragged", 48, ex, EXACT_VEC)
    add("exact-vec-d24", "f32", "nchw", True, "auto", "f32", "ragged", 24, ex, EXACT_VEC)
    add("exact-vec-bf16cells", "f32", "nchw", False, "exact", "bf16", "ragged", 48, ex, EXACT_VEC)
    add("exact-scalar-d24", "f32", "nchw", False, "auto", "f32", "odd", 24, ex, EXACT_SCALAR)
    # 16-bit operands
    add("pack-dma16-bf16", "bf16", "nchw", True, "auto", "bf16", "ragged", 96, rc, PACK_DMA16)
    add("pack-dma16-bf16-f32cells", "bf16", "nchw", True, "auto", "f32", "ragged", 96, rc,
        PACK_DMA16)
    add("pack-dma16-bf16-odd", "bf16", "nchw", True, "auto", "bf16", "odd", 96, rc, PACK_DMA16)
    add("pack-dma16-bf16-two", "bf16", "nchw", True, "auto", "bf16", "two", 96, rc, PACK_DMA16)
    add("pack-dma16-bf16-whole", "bf16", "nchw", True, "auto", "f32", "whole", 96, rc, PACK_DMA16)
    add("pack-dma16-f16", "f16", "nchw", True, "auto", "f32", "ragged", 96, rc, PACK_DMA16)
    add("pack-dma16-f16-f16cells", "f16", "nchw", True, "auto", "f16", "ragged", 96, rc,
        PACK_DMA16)
    add("dma16-nhwc-bf16", "bf16", "nhwc", False, "auto", "bf16", "ragged", 96, rc, DMA16_NHWC)
    add("dma16-nhwc-bf16-f32cells", "bf16", "nhwc", False, "auto", "f32", "ragged", 96, rc,
        DMA16_NHWC)
    add("dma16-nhwc-f16", "f16", "nhwc", False, "auto", "f32", "odd", 96, rc, DMA16_NHWC)
    add("dma16-nhwc-f16-f16cells", "f16", "nhwc", False, "auto", "f16", "ragged", 96, rc,
        DMA16_NHWC)
    add("bf16-q2", "bf16", "nchw", False, "auto", "bf16", "ragged", 96, rc, BF16_Q2)
    add("bf16-q2-f32cells", "bf16", "nchw", False, "auto", "f32", "ragged", 96, rc, BF16_Q2)
    add("bf16-q2-d48", "bf16", "nchw", False, "auto", "bf16", "ragged", 48, rc, BF16_Q2)
    add("bf16-scalar", "bf16", "nchw", False, "auto", "bf16", "odd", 96, rc, BF16_ONE)
    add("bf16-scalar-d48", "bf16", "nchw", False, "auto", "bf16", "odd", 48, rc, BF16_ONE)
    return t


REQUESTS = _requests()
# num_levels 1..3 (4 is every other request): the early returns between the staging barriers
LEVEL_REQUESTS = [r for r in REQUESTS if r.id in ("dma-nchw", "pack-dma16-bf16")]


# --------------------------------------------------------------------------- geometry
def level_shapes(H: int, W: int, L: int) -> list[tuple[int, int]]:
    return [(H >> lvl, W >> lvl) for lvl in range(L)]


def remainder_levels(H: int, W: int, L: int) -> list[tuple[int, bool, bool]]:
    """(level, odd rows, odd cols) of the levels a coarser level pools and whose
    floor-mode pooling leaves a remainder row and / or column."""
    return [(lvl, bool(h & 1), bool(w & 1)) for lvl, (h, w) in enumerate(level_shapes(H, W, L))
            if lvl + 1 < L and ((h & 1) or (w & 1))]


# --------------------------------------------------------------------------- number formats
def rne_bf16(x: np.ndarray) -> np.ndarray:
    """float32 values rounded to nearest even to bfloat16, as float32 (finite input)."""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return u.view(F32)


def rne_f16(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        return np.asarray(x).astype(np.float16).astype(F32)


def to_cells(v: np.ndarray, cells: str) -> np.ndarray:
    """float32 values as the cell type holds them (float64)."""
    if cells == "bf16":
        v = rne_bf16(v)
    elif cells == "f16":
        v = rne_f16(v)
    elif cells != "f32":
        raise ValueError(cells)
    return v.astype(np.float64)


# --------------------------------------------------------------------------- inputs
class Case:
    """Inputs of one build: fmaps [B, D, H, W] float32 holding values of the
    operand type.  Read-only."""

    def __init__(self, key, f1, f2, operand="f32"):
        self.key = key
        self.operand = operand
        self.f1, self.f2 = f1, f2
        self.B, self.D, self.H, self.W = f1.shape
        self.N = self.H * self.W
        self.div = np.sqrt(F32(self.D), dtype=F32)
        for a in (f1, f2):
            a.flags.writeable = False


_CASES: dict = {}
_REFS: dict = {}


def _wide_fmap(seed: int, B: int, D: int, H: int, W: int, dead: int) -> np.ndarray:
    """Pixel magnitudes 2^-12 .. 2^12, channel magnitudes 2^-18 .. 1 inside a pixel,
    about a tenth of the elements zero, every 11th pixel (from ``dead``) all zero."""
    N = H * W
    pix = np.exp2(np.floor(25 * dg.uniform(seed, B * N)) - 12).reshape(B, 1, N)
    chan = np.exp2(-np.floor(19 * dg.uniform(seed + 1, B * D * N))).reshape(B, D, N)
    z = dg.normal(seed + 2, B * D * N).reshape(B, D, N)
    z = np.where(z == 0, 1.0, z)
    keep = dg.uniform(seed + 3, B * D * N).reshape(B, D, N) >= 0.1
    f = z * chan * keep * pix
    f[:, :, np.arange(N) % 11 == dead] = 0.0
    return f.reshape(B, D, H, W).astype(F32)


def case(name: str, D: int, kind: str, operand: str = "f32") -> Case:
    key = (name, D, kind, operand)
    if key not in _CASES:
        B, H, W = CASES[name]
        seed = 7000 + 1000 * list(CASES).index(name) + 10 * D
        if kind == "uniform":
            f1, f2 = dg.fmap(seed, B, D, H, W, "fnet"), dg.fmap(seed + 1, B, D, H, W, "fnet")
        elif kind == "wide":
            f1, f2 = _wide_fmap(seed, B, D, H, W, 0), _wide_fmap(seed + 5, B, D, H, W, 3)
        else:
            raise ValueError(kind)
        if operand == "bf16":
            f1, f2 = rne_bf16(f1), rne_bf16(f2)
        elif operand == "f16":
            f1, f2 = rne_f16(f1), rne_f16(f2)
        elif operand != "f32":
            raise ValueError(operand)
        _CASES[key] = Case(key, f1, f2, operand)
    return _CASES[key]


def request_case(r: Request, kind: str) -> Case:
    return case(r.case, r.D, kind, r.operand)


# --------------------------------------------------------------------------- reference
def reference(c: Case, L: int = 4) -> dict:
    """ref, M: float64 pyramids (lists of [B*N, H_l, W_l]); Aq, At, Tq, Tt: level-0
    arrays [B*N, H, W] of the module docstring."""
    key = c.key + (L,)
    if key not in _REFS:
        B, D, N = c.B, c.D, c.N
        a1, a2 = np.abs(c.f1).astype(np.float64), np.abs(c.f2).astype(np.float64)
        m1, m2 = a1.reshape(B, D, N), a2.reshape(B, D, N)
        nz1, nz2 = (m1 != 0).astype(np.float64), (m2 != 0).astype(np.float64)
        shape = (B * N, c.H, c.W)
        _REFS[key] = {
            "ref": co.corr_pyramid(c.f1, c.f2, L, np.float64),
            "M": co.corr_pyramid(a1, a2, L, np.float64),
            "Aq": np.broadcast_to(m1.max(axis=1)[:, :, None], (B, N, N)).reshape(shape),
            "At": np.broadcast_to(m2.max(axis=1)[:, None, :], (B, N, N)).reshape(shape),
            "Tq": np.matmul(nz1.transpose(0, 2, 1), m2).reshape(shape),
            "Tt": np.matmul(m1.transpose(0, 2, 1), nz2).reshape(shape),
        }
    return _REFS[key]


# --------------------------------------------------------------------------- bounds
def nominal_magnitude(c: Case) -> np.ndarray:
    """Mn [B*N, H, W]: M with every non-zero float16 operand below 2^-14 taken as
    2^-14, the exponent the f16 MFMA aligns it by (module docstring)."""
    B, D, N = c.B, c.D, c.N
    n1, n2 = (np.where(f != 0, np.maximum(np.abs(f).astype(np.float64), 2.0 ** -14), 0.0)
              .reshape(B, D, N) for f in (c.f1, c.f2))
    return (np.matmul(n1.transpose(0, 2, 1), n2) / np.float64(c.div)).reshape(B * N, c.H, c.W)


def bound_level0(c: Case, family: str, t: dict) -> np.ndarray:
    """The float32 level-0 bound b0 of the family (module docstring)."""
    D, M = c.D, t["M"][0]
    div = np.float64(c.div)
    if family == "pair_scaled":
        return ((3 * D // 16 + 17) * U + 2.0 ** -21) * M + \
            (2.0 ** -38 * (1 + 2.0 ** -11) * (t["Aq"] * t["Tq"] + t["At"] * t["Tt"]) +
             D * 2.0 ** -76 * t["Aq"] * t["At"]) / div * (M > 0) + (M > 0) * 2.0 ** -149
    if family == "pair_unscaled":
        return ((D // 16 + 18) * U + (2 * D // 16 + 16) * U * 2.0 ** -10 + 2.0 ** -21) * M + \
            (2.0 ** -35 * (t["Tq"] + t["Tt"]) + D * 2.0 ** -50) / div * (M > 0) + \
            (M > 0) * 2.0 ** -149
    if family == "exact":
        return (8 * -(-D // 16) + 3) * U * M + (M > 0) * 2.0 ** -149
    if family == "rec16":
        b0 = (2 * -(-D // 32) + 17) * U * M + (M > 0) * 2.0 ** -149
        if c.operand == "f16":
            b0 = b0 + 17 * U * (nominal_magnitude(c) - M)
        return b0
    raise ValueError(family)


def bounds(c: Case, family: str, cells: str = "f32", L: int = 4) -> list[np.ndarray]:
    """Per level: (bound on |cell - ref|, float32 bound b_l underneath it)."""
    t = reference(c, L)
    out = []
    b = bound_level0(c, family, t)
    for lvl in range(L):
        if lvl:
            pb = co.avg_pool2x2(b)
            b = pb + 4 * U * (t["M"][lvl] + pb)
        _, e = np.frexp(np.abs(t["ref"][lvl]) + b)          # magnitude in [2^(e-1), 2^e)
        live = t["M"][lvl] > 0
        if cells == "bf16":
            full = b + live * np.ldexp(1.0, e - 9)
        elif cells == "f16":
            full = b + live * np.maximum(np.ldexp(1.0, e - 12), 2.0 ** -25)
        else:
            full = b
        out.append((full, b))
    return out


def check(c: Case, family: str, cells: str, got: list[np.ndarray], L: int = 4) -> list[float]:
    """Every cell of every level of ``got`` (float64 values of the cells) against
    the reference: the largest fraction of the bound used per level (inf where a
    cell breaks a rule outright); asserts nothing."""
    t = reference(c, L)
    fr = []
    for lvl, ((full, b), g) in enumerate(zip(bounds(c, family, cells, L), got)):
        ref, M = t["ref"][lvl], t["M"][lvl]
        g = np.asarray(g, dtype=np.float64).reshape(ref.shape)
        bad = np.isnan(g) | ((M == 0) & (g != 0))
        inf = np.isinf(g)
        if cells == "f16":
            must = np.abs(ref) - b >= F16_INF_FROM
            may = np.abs(ref) + b >= F16_INF_FROM
            bad |= must & ~(inf & (np.sign(g) == np.sign(ref)))
            bad |= inf & ~(may & (np.sign(g) == np.sign(ref)))
            ok_inf = inf & ~bad
        else:
            bad |= inf
            ok_inf = np.zeros_like(inf)
        with np.errstate(divide="ignore", invalid="ignore"):
            err = np.where(inf, 0.0, np.abs(np.where(inf, 0.0, g) - ref))
            use = np.where(full > 0, err / full, np.where(err > 0, np.inf, 0.0))
        use = np.where(ok_inf, 0.0, use)
        use = np.where(bad, np.inf, use)
        fr.append(float(use.max()))
    return fr


# --------------------------------------------------------------------------- emulation
def pixel_scale(m) -> np.ndarray:
    """``pixel_scale`` (corr_build.hip) restated: s = 14 - frexp exponent of the
    pixel's max, clamped to +-125; 0 for an all-zero pixel."""
    m = np.asarray(m, dtype=F32)
    _, e = np.frexp(m)
    return np.where(m > 0, np.clip(14 - e.astype(np.int64), -125, 125), 0)


def _r32(x: np.ndarray) -> np.ndarray:
    """One float32 rounding of float64 values, kept as float64."""
    return x.astype(F32).astype(np.float64)


def _f16(x: np.ndarray) -> np.ndarray:
    return x.astype(np.float16).astype(np.float64)


def pair_parts(x: np.ndarray, family: str, unscaled_split: bool = False):
    """(hi, lo, s, lo_exp) of fmap rows x [B, D, N] float32: x 2^s = hi + 2^lo_exp lo."""
    x = x.astype(np.float64)
    if family == "pair_scaled" and not unscaled_split:
        s = pixel_scale(np.abs(x).max(axis=1))[:, None, :]
    else:
        s = np.zeros((x.shape[0], 1, x.shape[2]), dtype=np.int64)
    X = np.ldexp(x, s)
    hi = _f16(X)
    if family == "pair_scaled":
        return hi, _f16(X - hi), s, 0
    return hi, _f16((X - hi) * 2048.0), s, -11


def subnormal_lo_share(c: Case) -> float:
    """Share of the non-zero elements whose scaled pair's low part lies inside
    float16's subnormal range (0 < |lo| < 2^-14)."""
    n = k = 0
    for f in (c.f1, c.f2):
        x = f.reshape(c.B, c.D, c.N)
        _, lo, _, _ = pair_parts(x, "pair_scaled")
        nz = x != 0
        n += int(nz.sum())
        k += int(((lo != 0) & (np.abs(lo) < 2.0 ** -14) & nz).sum())
    return k / n


def _level0(c: Case, family: str, flaw) -> np.ndarray:
    """[B, N, N] float32 level 0 of the family's arithmetic."""
    B, D, N = c.B, c.D, c.N
    x1, x2 = c.f1.reshape(B, D, N), c.f2.reshape(B, D, N)
    div = c.div
    if family in ("pair_scaled", "pair_unscaled"):
        us = flaw == "unscaled_split"
        qh, ql, sq, le = pair_parts(x1, family, us)
        th, tl, st, _ = pair_parts(x2, family, us)
        acc = np.zeros((B, N, N))
        acc2 = np.zeros((B, N, N))
        nst = D // 16
        for k in range(nst):
            sl = slice(16 * k, 16 * k + 16)
            a_h, a_l = qh[:, sl].transpose(0, 2, 1), ql[:, sl].transpose(0, 2, 1)
            cross = flaw != "no_lo" and not (flaw == "last_stage_cross" and k == nst - 1)
            if family == "pair_scaled":
                if cross and flaw != "one_cross":
                    acc = _r32(acc + a_h @ tl[:, sl])          # lo(target) hi(query)
                if cross:
                    acc = _r32(acc + a_l @ th[:, sl])
                acc = _r32(acc + a_h @ th[:, sl])
            else:
                if cross and flaw != "one_cross":
                    acc2 = _r32(acc2 + a_h @ tl[:, sl])
                if cross:
                    acc2 = _r32(acc2 + a_l @ th[:, sl])
                acc = _r32(acc + a_h @ th[:, sl])
        if family == "pair_unscaled":
            acc = _r32(acc2 * 2.0 ** le + acc)
        v = np.ldexp(acc, -(sq.transpose(0, 2, 1) + st)).astype(F32)
    elif family == "exact":
        a, b = x1.astype(np.float64), x2.astype(np.float64)
        acc = np.zeros((B, N, N))
        for k in range(0, D, 2):
            acc = _r32(acc + a[:, k:k + 2].transpose(0, 2, 1) @ b[:, k:k + 2])
        v = acc.astype(F32)
    elif family == "rec16":
        a, b = x1.astype(np.float64), x2.astype(np.float64)
        acc = np.zeros((B, N, N))
        for k in range(0, D, 16):
            acc = _r32(acc + a[:, k:k + 16].transpose(0, 2, 1) @ b[:, k:k + 16])
        v = acc.astype(F32)
    else:
        raise ValueError(family)
    return v / div                              # float32 division


def _pool32(x: np.ndarray, ceil: bool) -> np.ndarray:
    """The epilogue's float32 pooling; ``ceil``: the flawed form whose last window
    of an odd dimension takes the remainder row / column in (shifted by one)."""
    H, W = x.shape[-2:]
    Ho, Wo = H // 2, W // 2
    r0, c0 = 2 * np.arange(Ho), 2 * np.arange(Wo)
    if ceil and H & 1:
        r0[-1] += 1
    if ceil and W & 1:
        c0[-1] += 1
    g = lambda dr, dc: x[..., (r0 + dr)[:, None], (c0 + dc)[None, :]]   # noqa: E731
    with np.errstate(invalid="ignore", over="ignore"):     # inf cells of a flawed float16 chain
        return (((g(0, 0) + g(0, 1)) + g(1, 0)) + g(1, 1)) * F32(0.25)


def emulate(c: Case, family: str, cells: str = "f32", L: int = 4, flaw=None) -> list[np.ndarray]:
    """The pyramid of the family's arithmetic as float64 values of ``cells``.
    Flaws: ``one_cross`` (the lo(target) hi(query) product is never added),
    ``last_stage_cross`` (no cross product in the final K stage), ``no_lo``,
    ``unscaled_split`` (the pair taken without the per-pixel scale), ``pool_of_rounded``
    (a level pooled from the rounded cells of the one above), ``pool_ceil``,
    ``partial_page_shift`` (the queries of a last, partial 128-query page read
    the neighbouring target column)."""
    if flaw is not None and flaw not in FLAWS:
        raise ValueError(flaw)
    v = _level0(c, family, flaw).reshape(c.B * c.N, c.H, c.W)
    assert v.dtype == F32
    if flaw == "partial_page_shift" and c.N % PQ:
        v = v.reshape(c.B, c.N, c.H, c.W).copy()
        first = c.N // PQ * PQ
        v[:, first:] = np.roll(v[:, first:], -1, axis=3)
        v = v.reshape(c.B * c.N, c.H, c.W)
    out = []
    for lvl in range(L):
        if lvl:
            v = _pool32(v, flaw == "pool_ceil")
        out.append(to_cells(v, cells))
        if flaw == "pool_of_rounded":
            v = out[-1].astype(F32)
    return out
