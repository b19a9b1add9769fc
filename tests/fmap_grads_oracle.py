"""float64 oracle, per-element bounds and host emulation of the fused
fmap-gradient GEMMs of ``csrc/corr_backward.hip`` (``dxr_fmap_grads``,
``dxr_fmap_grads_bounded``).  numpy and ``oracle.corr_oracle`` only: no code
under test.

The operation.  G is a gradient pyramid (level l: [B*N, H_l, W_l], N = H W).
Folded down the pooling chain (``oracle.corr_pyramid_backward``'s fold: level l
receives a quarter of level l + 1's total, the floor-mode remainder row and
column receive nothing) and divided by the float32 sqrt(D) it is dV [B, N, N];

    dF1[b, d, q] = sum_t F2[b, d, t] dV[b, q, t]      (K runs over targets)
    dF2[b, d, t] = sum_q F1[b, d, q] dV[b, q, t]      (K runs over queries)

Per output element ``gemm_terms`` returns the float64 value ``ref`` and what its
error is measured against:

    A    the same sum over |F| and the fold of |G| (no cancellation)
    n    the number of k with F != 0 and dV != 0 (zero products add no error)
    SF   sum of |F[d, k]| over the k where dV != 0
    SV   sum of |dV[., k]| over the k where F[d, k] != 0 (the fold of |G|)

The bound of the f16-pair form (``bound_pair``)
-----------------------------------------------
Contract (``dxr::split8_f16_prescaled``, csrc/mfma_operands.h; file comment of
corr_backward.hip, DESIGN 3.5 rounds 4 and 5 (i)): an operand x runs as hi + lo of X = x 2^s, hi = RNE_f16(X), lo = RNE_f16(X - hi),
with s chosen by ``scale_for`` from a bound m on |x|: m < 2^e (frexp), s = 14 - e
clamped to +-125, so |X| < 2^14.  ``bf_of`` / ``bv_of`` restate that and return
the power of two the scale stands for, P = 2^(14 - s): one per channel and pair
for the fmap (m = the channel's max |x|), one for all of dV
(m = max(slots) * vfac, vfac = 1.34f / |divisor|, both float32).

 * Operand error.  float16 has 11 significand bits and subnormal spacing 2^-24:
   |X - hi| <= 2^-11 |X| (or 2^-25 below 2^-14), the remainder is exact in
   float32, |r - lo| <= 2^-11 |r| or 2^-25.  So |X - hi - lo| <= 2^-22 |X| + 2^-25,
   and in x's units  e(x) <= 2^-22 |x| + 2^-39 P  -- the stated contract.
 * A product a t is replaced by ah th + ah tl + al th.  The difference is
   al tl + e(a) t + (ah + al) e(t), with |al|, |tl| <= 2^-11 (1 + 2^-11) of their
   values: to first order
       3 2^-22 |a| |t|  +  2^-39 (PF |t| + PV |a|).
   Both constants are rounded up to the next power of two, 4 2^-22 and 2^-38:
   that covers the second-order terms, and leaves an arithmetic that meets the
   contract exactly at no more than about half of the bound, which
   tests/test_fmap_grads_bound_cpu.py asserts of the emulation below.  A zero
   operand splits into zeros, its products are exactly zero: only k with both
   operands non-zero count, which is why SF and SV are masked sums.
 * The fold computes a dV element in float32 with L - 1 steps g + t / 4 and one
   division (or an exact multiplication): at most L roundings; the issue's count
   L + 2 is kept.  Each is 2^-24 relative to the fold of |G| (the 1/4 factors are
   exact), so (L + 2) 2^-24 A in the result.  Where G is so small that the fold
   runs on float32 subnormals each step errs by 2^-150 absolute instead:
   (L + 2) 2^-150 SF.
 * Accumulation.  The f16 products are exact in float32.  A k-step issues three
   MFMAs into the float32 accumulator (lo hi, hi lo, hi hi); with one rounding
   per non-zero product at worst that is 3 n roundings of 2^-24 relative to the
   partial sum of magnitudes (<= A).  K split in S chunks adds S - 1 roundings in
   ``chunk_sum_kernel``.  Un-scaling is an exact ldexp unless the result is a
   float32 subnormal; every chunk's partial sum is un-scaled and stored on its
   own, so S roundings to the subnormal grid: S 2^-150.

    bound = c_rel(n) A + 2^-38 (PF[d] SV + PV SF) + (L + 2) 2^-150 SF
            + half a float32 ulp of (|ref| + the above) + S 2^-150
    c_rel(n) = 4 2^-22 + (3 n + S - 1 + L + 2) 2^-24

The bound of the six-product form (``bound_six``)
-------------------------------------------------
``dxr::split8_bf16<GUARD_INF_AND_RANGE>`` (csrc/mfma_operands.h): x = hi + mid + lo with hi, mid RNE to bfloat16 (8
significand bits) and lo the top 16 bits of the last remainder.  The remainder
after two 8-bit roundings of a 24-bit significand has at most 8 bits, so lo is
exact in the normal range; 2^-25 |x| is allowed per operand all the same (what
the truncation would lose if it had more).  |mid| <= 2^-9 |x|, |lo| <= 2^-17 |x|;
the three dropped products (mid lo, lo mid, lo lo) are below 2^-25 |a| |t|.  Six
MFMAs per k-step.  No scales, so no absolute term but the fold's:

    c_rel(n) = 2 2^-25 + 2^-25 + (6 n + S - 1 + L + 2) 2^-24
    bound = c_rel(n) A + (L + 2) 2^-150 SF + half an ulp + S 2^-150

No constant here comes from a measured error of the kernels.
"""
from __future__ import annotations

import math

import numpy as np

import datagen as dg
from oracle import corr_oracle as co

F32 = np.float32
PQ, TH, TW, DS = 128, 8, 16, 256           # page queries, tile rows, tile cols, channel slab
SPARSITY = (1, 2, 5, 16, 100)              # non-zero cells per level row, cycled over queries
FLAWS = ("flush", "no_lo_dv", "no_lo_fmap", "no_lohi", "floor_mask")

# (B, D, H, W, L) of tests/test_gpu_fmap_grads_per_element.py, and what each is there for
SHAPES = [
    (1, 32, 8, 16, 2),      # one query block, one tile: no K split in either kernel
    (1, 32, 9, 17, 1),      # one level, ragged tile and query block
    (2, 64, 23, 37, 3),     # odd at every level, two pairs
    (1, 288, 16, 24, 4),    # two 256-channel slabs, the second partial
    (1, 256, 24, 40, 4),    # 7.5 query blocks, K split
]
EDGE_SHAPE = SHAPES[2]


def shape_case(shape, kind: str) -> "Case":
    return case(4100 + 100 * SHAPES.index(shape), *shape, kind)


# --------------------------------------------------------------------------- geometry
def level_shapes(H: int, W: int, L: int) -> list[tuple[int, int]]:
    return [(H >> lvl, W >> lvl) for lvl in range(L)]


def remainder_levels(H: int, W: int, L: int) -> list[tuple[int, bool, bool]]:
    """(level, odd rows, odd cols) of the levels that a coarser level pools and
    whose floor-mode pooling leaves a remainder row and / or column."""
    return [(lvl, bool(h & 1), bool(w & 1)) for lvl, (h, w) in enumerate(level_shapes(H, W, L))
            if lvl + 1 < L and ((h & 1) or (w & 1))]


def k_chunks(B: int, D: int, H: int, W: int, kt: bool) -> int:
    """``set_kernel``'s split rule restated: the K chunks S of the dF1 GEMM
    (``kt``: n blocks are query blocks, k blocks level-0 tiles) or the dF2 GEMM."""
    qt = -(-(H * W) // PQ)
    tiles = -(-H // TH) * -(-W // TW)
    nblk, kbt = (qt, tiles) if kt else (tiles, qt)
    units = nblk * B * -(-D // DS)
    S = 1 if units >= 256 else 256 // units
    return min(S, kbt)


# --------------------------------------------------------------------------- scales
def scale_for(m) -> np.ndarray:
    """``scale_for`` restated: s = 14 - frexp exponent of m, clamped to +-125; 0
    for m == 0.  m: finite float32 >= 0."""
    m = np.asarray(m, dtype=F32)
    _, e = np.frexp(m)
    s = np.clip(14 - e.astype(np.int64), -125, 125)
    return np.where(m > 0, s, 0)


def bf_of(f: np.ndarray) -> np.ndarray:
    """[B, D] float64: the power of two 2^(14 - s) each channel's scale stands for."""
    B, D = f.shape[:2]
    return np.ldexp(1.0, 14 - scale_for(np.abs(f).reshape(B, D, -1).max(axis=2)))


def dv_scale(slot_max, div) -> int:
    vfac = F32(1.34) / np.abs(F32(div))
    return int(scale_for(F32(slot_max) * vfac))


def bv_of(slot_max, div) -> float:
    return math.ldexp(1.0, 14 - dv_scale(slot_max, div))


# --------------------------------------------------------------------------- inputs
class Case:
    """Inputs of one call: fmaps [B, D, H, W] float32, gradient levels
    [B*N, H_l, W_l] float32, the float32 divisor sqrt(D).  Read-only."""

    def __init__(self, key, f1, f2, G):
        self.key = key
        self.f1, self.f2, self.G = f1, f2, G
        self.B, self.D, self.H, self.W = f1.shape
        self.L = len(G)
        self.N = self.H * self.W
        self.div = np.sqrt(F32(self.D), dtype=F32)
        for a in (f1, f2, *G):
            a.flags.writeable = False

    @property
    def gmax(self) -> float:
        return max(float(np.abs(g).max()) for g in self.G)


_CASES: dict = {}
_TERMS: dict = {}


def case(seed: int, B: int, D: int, H: int, W: int, L: int, kind: str) -> Case:
    key = (seed, B, D, H, W, L, kind)
    if key not in _CASES:
        _CASES[key] = Case(key, *(_uniform if kind == "uniform" else _wide)(seed, B, D, H, W, L))
    return _CASES[key]


def _uniform(seed, B, D, H, W, L):
    """What tests/test_gpu_backward.py feeds: fnet-like fmaps, N(0, 1) on every
    cell of every level."""
    if L < 1:
        raise ValueError(L)
    f1, f2 = dg.fmap(seed, B, D, H, W, "fnet"), dg.fmap(seed + 1, B, D, H, W, "fnet")
    G = [dg.normal(seed + 10 + lvl, B * H * W * h * w).reshape(B * H * W, h, w).astype(F32)
         for lvl, (h, w) in enumerate(level_shapes(H, W, L))]
    return f1, f2, G


def _wide_fmap(seed, B, D, H, W, zero_mod):
    k = np.floor(17 * dg.uniform(seed, B * D)).reshape(B, D, 1, 1) - 8          # -8..8
    f = dg.normal(seed + 1, B * D * H * W).reshape(B, D, H, W) * np.exp2(k)
    pix = np.floor(dg.uniform(seed + 2, B) * H * W).astype(np.int64)
    for b in range(B):                                   # one outlier pixel per pair
        f[b, :, pix[b] // W, pix[b] % W] *= 2.0 ** 9
    f[:, np.arange(D) % 13 == zero_mod] = 0.0            # a few channels all zero
    return f.astype(F32)


def _wide(seed, B, D, H, W, L):
    f1, f2 = _wide_fmap(seed, B, D, H, W, 5), _wide_fmap(seed + 3, B, D, H, W, 7)
    BN = B * H * W
    q = np.arange(BN)
    scale = np.exp2(-(q % 25).astype(np.float64))
    dead = q % 11 == 0                                   # an invalid pixel: zero on every level
    rem = {lvl: (oh, ow) for lvl, oh, ow in remainder_levels(H, W, L)}
    G = []
    for lvl, (h, w) in enumerate(level_shapes(H, W, L)):
        cells = h * w
        cnt = np.minimum(np.asarray(SPARSITY)[q % len(SPARSITY)], cells)
        u = dg.uniform(seed + 20 + lvl, BN * cells).reshape(BN, cells)
        thr = np.sort(u, axis=1)[q, cnt - 1]
        mask = u <= thr[:, None]
        oh, ow = rem.get(lvl, (False, False))
        pick = q % 3 == 1
        if oh:                                           # the remainder row ...
            mask[q[pick], (h - 1) * w + (7 * q[pick]) % w] = True
        if ow:                                           # ... and column hold gradient
            mask[q[pick], ((5 * q[pick]) % h) * w + w - 1] = True
        v = dg.normal(seed + 30 + lvl, BN * cells).reshape(BN, cells)
        v = np.where(v == 0, 1.0, v) * mask * scale[:, None]
        v[dead] = 0.0
        G.append(v.reshape(BN, h, w).astype(F32))
    return f1, f2, G


def rescaled(c: Case, g_exp: int = 0, f_exp: int = 0, zero_pair=None) -> Case:
    """``c`` with G times 2^g_exp and the fmaps times 2^f_exp, rounded to float32
    (the float32 arrays are the inputs: what underflows is part of the case);
    ``zero_pair``: that pair's G all zero."""
    key = c.key + ("rescaled", g_exp, f_exp, zero_pair)
    if key not in _CASES:
        G = [np.ldexp(g, g_exp).astype(F32) for g in c.G]
        if zero_pair is not None:
            for g in G:
                g[zero_pair * c.N:(zero_pair + 1) * c.N] = 0
        _CASES[key] = Case(key, np.ldexp(c.f1, f_exp).astype(F32),
                           np.ldexp(c.f2, f_exp).astype(F32), G)
    return _CASES[key]


# --------------------------------------------------------------------------- reference
def fold(levels, floor_mask: bool = False) -> np.ndarray:
    """oracle.corr_pyramid_backward's fold in float64, not yet divided.
    ``floor_mask``: the flawed fold that lets the pooled total reach the
    remainder row and column (they copy their neighbours' share)."""
    tot = levels[-1].astype(np.float64)
    for lvl in range(len(levels) - 2, -1, -1):
        h, w = levels[lvl].shape[-2:]
        up = co.avg_pool2x2_backward(tot, (h, w))
        if floor_mask:
            if h & 1:
                up[..., h - 1, :] = up[..., h - 2, :]
            if w & 1:
                up[..., :, w - 1] = up[..., :, w - 2]
        tot = levels[lvl].astype(np.float64) + up
    return tot


def gemm_terms(f1, f2, levels, mag_levels) -> dict:
    """{"df1": t, "df2": t}, t = dict(ref, A, n, SF, SV) as [B, D, H, W] float64
    (see the module docstring).  ``levels``: the gradient pyramid; ``mag_levels``:
    the magnitudes errors are relative to (|G|, or the lookup backward's M)."""
    B, D, H, W = f1.shape
    N = H * W
    div = np.float64(np.sqrt(F32(D), dtype=F32))
    r1, r2 = co.corr_pyramid_backward(f1, f2, levels)
    va = (fold(mag_levels) / div).reshape(B, N, N)
    nzv = (va != 0).astype(np.float64)
    out = {}
    for name, ref, f, tr in (("df1", r1, f2, True), ("df2", r2, f1, False)):
        a = np.abs(f.reshape(B, D, N).astype(np.float64))
        nza = (a != 0).astype(np.float64)
        v, z = (va.transpose(0, 2, 1), nzv.transpose(0, 2, 1)) if tr else (va, nzv)
        out[name] = {"ref": ref, "A": (a @ v).reshape(ref.shape), "n": (nza @ z).reshape(ref.shape),
                     "SF": (a @ z).reshape(ref.shape), "SV": (nza @ v).reshape(ref.shape)}
    return out


def reference(c: Case) -> dict:
    if c.key not in _TERMS:
        _TERMS[c.key] = gemm_terms(c.f1, c.f2, c.G, [np.abs(g) for g in c.G])
    return _TERMS[c.key]


# --------------------------------------------------------------------------- bounds
def _half_ulp32(x: np.ndarray) -> np.ndarray:
    return 0.5 * np.spacing(np.abs(x).astype(F32)).astype(np.float64)


def _finish(t, b0, S):
    return b0 + _half_ulp32(np.abs(t["ref"]) + b0) + S * 2.0 ** -150


def bound_pair(t: dict, f: np.ndarray, slot_max, div, L: int, S: int) -> np.ndarray:
    """Per-element bound of the f16-pair form.  ``t``: one side of gemm_terms;
    ``f``: that side's fmap operand (fmap2 for df1); ``slot_max``: the largest
    bound slot the call is given."""
    c_rel = 4 * 2.0 ** -22 + (3 * t["n"] + (S - 1) + L + 2) * 2.0 ** -24
    pf = bf_of(f)[:, :, None, None]
    b0 = c_rel * t["A"] + 2.0 ** -38 * (pf * t["SV"] + bv_of(slot_max, div) * t["SF"]) + \
        (L + 2) * 2.0 ** -150 * t["SF"]
    return _finish(t, b0, S)


def bound_six(t: dict, L: int, S: int) -> np.ndarray:
    """Per-element bound of the six-product bf16 form."""
    c_rel = 3 * 2.0 ** -25 + (6 * t["n"] + (S - 1) + L + 2) * 2.0 ** -24
    return _finish(t, c_rel * t["A"] + (L + 2) * 2.0 ** -150 * t["SF"], S)


def fraction(err: np.ndarray, bound: np.ndarray) -> float:
    """The largest err / bound; inf where an error exceeds a zero bound."""
    with np.errstate(divide="ignore", invalid="ignore"):
        use = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(use.max())


# --------------------------------------------------------------------------- emulation
def _pair16(x: np.ndarray, s) -> tuple[np.ndarray, np.ndarray]:
    """Mirrors ``dxr::split8_f16_prescaled`` (csrc/mfma_operands.h): (hi, lo) of
    x 2^s as float64 values of numpy float16 roundings."""
    X = np.ldexp(x.astype(np.float64), s)
    hi = X.astype(np.float16).astype(np.float64)
    lo = (X - hi).astype(np.float16).astype(np.float64)
    return hi, lo


def subnormal_share(c: Case, slot_max=None) -> tuple[float, float]:
    """Shares of the non-zero fmap and dV operand elements whose scaled f16 pair
    has a part inside the float16 subnormal range (0 < |part| < 2^-14)."""
    def share(parts, nz):
        sub = np.zeros(nz.shape, dtype=bool)
        for p in parts:
            sub |= (p != 0) & (np.abs(p) < 2.0 ** -14)
        return float(sub[nz].mean())
    f = np.concatenate([c.f1, c.f2]).reshape(2 * c.B, c.D, c.N)
    sf = scale_for(np.abs(f).max(axis=2))[:, :, None]
    t = (fold(c.G) / np.float64(c.div)).astype(F32)
    ev = dv_scale(c.gmax if slot_max is None else slot_max, c.div)
    return share(_pair16(f, sf), f != 0), share(_pair16(t, ev), t != 0)


def emulate(c: Case, flaw: str | None = None, slot_max=None) -> tuple[np.ndarray, np.ndarray]:
    """(dF1, dF2) of the f16-pair arithmetic on the host: the float64 fold rounded
    once to float32, hi = RNE_f16 of the scaled value, lo = RNE_f16 of the
    remainder, the three products, float64 sums, exact un-scaling.  Flaws:
    ``flush`` (float16 subnormal parts read as zero), ``no_lo_dv`` / ``no_lo_fmap``
    (that operand's low part zero), ``no_lohi`` (the lo(fmap) hi(dV) product left
    out: with three products the same sum as ``no_lo_fmap``), ``floor_mask``."""
    if flaw is not None and flaw not in FLAWS:
        raise ValueError(flaw)
    B, D, N = c.B, c.D, c.N
    t = (fold(c.G, flaw == "floor_mask") / np.float64(c.div)).astype(F32).reshape(B, N, N)
    ev = dv_scale(c.gmax if slot_max is None else slot_max, c.div)
    th, tl = _pair16(t, ev)
    if flaw == "no_lo_dv":
        tl = np.zeros_like(tl)
    outs = []
    for f, tr in ((c.f2, True), (c.f1, False)):
        f = f.reshape(B, D, N)
        s = scale_for(np.abs(f).max(axis=2))[:, :, None]
        ah, al = _pair16(f, s)
        if flaw == "no_lo_fmap":
            al = np.zeros_like(al)
        parts = [ah, al, th, tl]
        if flaw == "flush":
            parts = [np.where(np.abs(p) < 2.0 ** -14, 0.0, p) for p in parts]
        xh, xl, yh, yl = parts
        if tr:
            yh, yl = yh.transpose(0, 2, 1), yl.transpose(0, 2, 1)
        acc = xh @ yl + xh @ yh
        if flaw != "no_lohi":
            acc = xl @ yh + acc
        outs.append(np.ldexp(acc, -(s + ev)).reshape(B, D, c.H, c.W))
    return outs[0], outs[1]
