"""float64 oracle, per-element bounds and host emulation of the GEMM of the
lookup fused with convc1 (``corr_lookup_conv1x1_h2_kernel`` in
``csrc/corr_lookup.hip``, reached through ``CorrBlock.lookup_conv1x1``).  numpy
and ``oracle/`` only: no code under test.

The operation.  x[c, q] are the lookup's samples of query q (float32, the
unfused lookup's bit for bit), w[o, c] the convolution weight, b[o] the bias:

    ref[o, q] = b[o] + sum_c w[o, c] x[c, q]                      (float64)
    M0[o, q]  = sum_c |w[o, c]| |x[c, q]|,     M = |b[o]| + M0    (no cancellation)

``terms`` returns them with the three sums the bounds need.

The kernel (what the bounds restate)
------------------------------------
One workgroup owns QB = 32 consecutive queries of one batch item.  Channels are
padded with zeros to cin_pad (whole k steps of 16); a wave owns 32 output rows
and runs the k steps in order, one v_mfma_f32_32x32x16 per product and step.
Grids of at most 256 workgroups run 1024 threads: waves 8..15 take the second
half of the k steps (KSPLIT = 2) and their sums are added to the first half's
through LDS; larger grids run 512 threads, KSPLIT = 1.  ``ksplit_of`` restates
the rule.

``dxr::split8_f16`` (csrc/mfma_operands.h): an operand v (weight or sample) runs
as hi = RNE_f16(v) and
lo = RNE_f16((v - hi) 2048), both subtraction and scaling exact in float32.
Per k step  acc2 += lo_w hi_x,  acc2 += hi_w lo_x,  acc += hi_w hi_x  in float32;
then acc = fmaf(acc2, 2^-11, acc), the KSPLIT add, the bias add.  A workgroup
that sees a non-finite sum repeats its GEMM on
``dxr::split8_bf16<GUARD_INF_AND_RANGE>`` (below).

The bound of the f16-pair form (``bound_pair``)
-----------------------------------------------
float16 has 11 significand bits, smallest normal 2^-14, subnormal spacing
2^-24.  For an operand of magnitude a > 0

    d(a) = 2^-11 a  if a >= 2^-14, else 2^-25          bounds |v - hi|
    e(a) = max(2^-11 d(a), 2^-36)                      bounds |v - hi - lo / 2048|

(the rounding of lo, relative 2^-11 of a value <= 2048 d(a) or 2^-25 absolute,
carried back through / 2048; d(a) >= 2^-25 makes the max redundant, it is kept
as stated).  A zero operand splits into zeros and its products are exactly
zero: d(0) = e(0) = 0.  With dw = w - hi_w, dx = x - hi_x:

    w x - (hi_w hi_x + hi_w lo_x / 2048 + lo_w hi_x / 2048)
        = dw dx + hi_w (dx - lo_x / 2048) + (dw - lo_w / 2048) hi_x

so to first order, per channel,
    d(|w|) d(|x|)      the dropped lo lo product
  + |w| e(|x|)         the rounding of the sample's lo
  + e(|w|) |x|         the rounding of the weight's lo.
In the normal range each is 2^-22 |w| |x|: 3 2^-22 M0 in all.

Every f16 x f16 product is exact in float32 (22 bits).  Float32 roundings of one
output, each at most 2^-24 of the sum of magnitudes so far (<= M):
  * acc: one per real channel at worst (a padded channel adds an exact zero): cin
  * acc2: 2 cin, but of a sum that counts 2^-11 x (|lo_w hi_x| + |hi_w lo_x|) / 2048
    <= 2^-10 (1 + 2^-11) M0: cin 2^-9 (1 + 2^-11) roundings' worth, < 1 for every
    cin the kernel takes (cin_pad <= 336): counted as 1
  * the fmaf of acc2 into acc: 1
  * the KSPLIT add: KSPLIT - 1
  * the bias add: 1 with a bias
    gamma = cin + 2 + (KSPLIT - 1) + (1 with a bias)         (at most cin + 4)

    bound = sum_c [d(|w|) d(|x|) + e(|w|) |x| + |w| e(|x|)] + gamma 2^-24 M

Second-order terms (|hi_w| <= |w| + d(|w|) in the two lo terms, the compounding
of gamma roundings) are 2^-10 of the first term and about 2^-31 M: in the normal
range the unit counted for acc2 (worth 0.63 at cin = 324) covers them; they are
not added.  No term is needed for float32 underflow: a non-zero f16 part is at
least 2^-24, so every product and partial sum is a multiple of 2^-59.

The bound of the bf16 three-way fallback (``bound_six``)
--------------------------------------------------------
``dxr::split8_bf16<GUARD_INF_AND_RANGE>`` (csrc/mfma_operands.h):
hi = RNE_bf16(v), mid = RNE_bf16(v - hi), lo = the top 16 bits
of v - hi - mid.  bfloat16 has 8 significand bits: |v - hi| <= 2^-8 |v| with at
most 16 significant bits left, |v - hi - mid| <= 2^-16 |v| with at most 8, so lo
is exact and v = hi + mid + lo while all three are bf16 normals (|v| >= 2^-103:
the callers keep fallback operands at 2^-100 or above; nothing is claimed
below).  Six of the nine products are formed (mid mid, lo hi, hi lo, mid hi,
hi mid, hi hi), each exact in float32 (16 bits); the dropped three are at most
    |mid_w lo_x| + |lo_w mid_x| + |lo_w lo_x| <= (2 2^-24 + 2^-32) |w| |x|.
Six accumulations per channel into one accumulator, of sums of magnitudes at
most (1 + 2^-8 + 2^-16)^2 M0 < (1 + 2^-6) M: gamma6 = 6 cin + (KSPLIT - 1) +
(1 with a bias).  Operands down to 2^-100 put products and partial sums into
float32's subnormal range, where a rounding is absolute (the matrix cores keep
subnormal accumulators): 2^-149 each.

    bound6 = (2^-23 + 2^-32) M0 + gamma6 2^-24 (1 + 2^-6) M + gamma6 2^-149

No constant here comes from a measured error of the kernel.
"""
from __future__ import annotations

import numpy as np

import datagen as dg
import oracle

F32 = np.float32
QB = 32                                    # queries per workgroup
F16_MIN_NORMAL = 2.0 ** -14
F16_LIMIT = 65520.0                        # the smallest magnitude that rounds to inf in float16
X_TOP = 65519.0                            # the largest float32 that rounds to a finite float16
FLAWS = ("flush", "drop", "scale", "unpadded", "no_fallback")
CONFIGS = [(4, 4), (4, 3), (2, 4), (1, 3)]             # (levels, radius)
ZERO_Q, TOP_Q = 21, 12                                 # columns of the "wide" sample builder


def cin_of(levels: int, radius: int) -> int:
    return levels * (2 * radius + 1) ** 2


def cin_pad(cin: int) -> int:
    return (cin + 15) // 16 * 16


def ksplit_of(B: int, N: int) -> int:
    """``launch_lookup_conv1x1_r``'s rule: up to 256 workgroups run the
    1024-thread form, whose wave halves split the k steps."""
    return 2 if B * (-(-N // QB)) <= 256 else 1


# --------------------------------------------------------------------------- inputs
def _binade(seed: int, n: int, lo: int, hi: int) -> np.ndarray:
    """2^e, integer e uniform in [lo, hi]."""
    return np.exp2(np.floor((hi - lo + 1) * dg.uniform(seed, n)) + lo)


def unit_weights(seed: int, cout: int, cin: int):
    """What today's max-norm tests feed: w ~ N(0, 1) / sqrt(cin), bias ~ N(0, 1) / 2."""
    w = dg.normal(seed, cout * cin).reshape(cout, cin) / np.sqrt(cin)
    return w.astype(F32), (0.5 * dg.normal(seed + 1, cout)).astype(F32)


def wide_weights(seed: int, cout: int, cin: int):
    """N(0, 1) 2^e, e in [-30, 2]; the first 8 rows (weights and bias) a further 2^-20."""
    w = dg.normal(seed, cout * cin) * _binade(seed + 1, cout * cin, -30, 2)
    b = dg.normal(seed + 2, cout) * _binade(seed + 3, cout, -30, 2)
    w = w.reshape(cout, cin)
    w[:8] *= 2.0 ** -20
    b[:8] *= 2.0 ** -20
    return w.astype(F32), b.astype(F32)


def unit_samples(seed: int, cin: int, nq: int) -> np.ndarray:
    return dg.normal(seed, cin * nq).reshape(cin, nq).astype(F32)


def wide_samples(seed: int, cin: int, nq: int) -> np.ndarray:
    """[cin, nq]: N(0, 1) 2^e, e in [-30, 10]; about 10 % exact zeros; the first 8
    queries of every workgroup a further 2^-20; column ZERO_Q all zero; one sample
    of exactly 65519 in column TOP_Q."""
    assert nq > max(ZERO_Q, TOP_Q)
    x = dg.normal(seed, cin * nq) * _binade(seed + 1, cin * nq, -30, 10)
    x[dg.uniform(seed + 2, cin * nq) < 0.1] = 0.0
    x = x.reshape(cin, nq)
    x[:, np.arange(nq) % QB < 8] *= 2.0 ** -20
    x[:, ZERO_Q] = 0.0
    x[cin // 2, TOP_Q] = X_TOP
    x = x.astype(F32)
    assert np.abs(x).max() == F32(X_TOP)
    return x


def inputs(kind: str, seed: int, cout: int, cin: int, nq: int):
    """(w [cout, cin], bias [cout], x [cin, nq]) float32 of one batch item."""
    if kind == "unit":
        return (*unit_weights(seed, cout, cin), unit_samples(seed + 10, cin, nq))
    if kind == "wide":
        return (*wide_weights(seed, cout, cin), wide_samples(seed + 10, cin, nq))
    raise ValueError(kind)


def workgroups(nq: int, n_item: int | None = None) -> list[slice]:
    """The column ranges of the workgroups of ``nq`` queries, ``n_item`` per batch
    item (a workgroup never spans two items; an item's last one may be ragged)."""
    n_item = nq if n_item is None else n_item
    return [slice(s, min(s + QB, i + n_item)) for i in range(0, nq, n_item)
            for s in range(i, i + n_item, QB)]


def with_overflowing_weight(w: np.ndarray, x: np.ndarray, n_item: int | None = None, row: int = 9):
    """(w', c): ``w`` with 1e5 (inf in float16) at [row, c], c the first channel
    that has a non-zero sample in every workgroup of ``x`` [cin, nq]."""
    nz = x != 0
    groups = [nz[:, g].any(axis=1) for g in workgroups(x.shape[1], n_item)]
    c = int(np.flatnonzero(np.logical_and.reduce(groups))[0])
    w = w.copy()
    w[row, c] = 1e5
    return w, c


# --------------------------------------------------------------------------- reference and bounds
def _d(a: np.ndarray) -> np.ndarray:
    return np.where(a >= F16_MIN_NORMAL, 2.0 ** -11 * a, np.where(a > 0, 2.0 ** -25, 0.0))


def _e(a: np.ndarray) -> np.ndarray:
    return np.where(a > 0, np.maximum(2.0 ** -11 * _d(a), 2.0 ** -36), 0.0)


def e_of(a: np.ndarray) -> np.ndarray:
    """e(|a|): what the one-hot test allows between an output and its sample."""
    return _e(np.abs(np.asarray(a, dtype=np.float64)))


def terms(w: np.ndarray, x: np.ndarray) -> dict:
    """``w`` [cout, cin], ``x`` [cin, Q] float32 -> float64 [cout, Q] arrays: ref0
    (no bias, ``oracle.motion_conv1x1``), M0 and ``split``, the sum over channels
    of d(|w|) d(|x|) + e(|w|) |x| + |w| e(|x|)."""
    cin, Q = x.shape
    ref0 = oracle.motion_conv1x1(x.reshape(1, cin, 1, Q), w, None, relu=False).reshape(-1, Q)
    aw, ax = np.abs(w.astype(np.float64)), np.abs(x.astype(np.float64))
    return {"ref0": ref0, "M0": aw @ ax, "split": _d(aw) @ _d(ax) + _e(aw) @ ax + aw @ _e(ax),
            "cin": cin}


def rows(t: dict, cout: int) -> dict:
    """The terms of the first ``cout`` rows of the weight."""
    return {k: (v if k == "cin" else v[:cout]) for k, v in t.items()}


def _bias64(t: dict, bias) -> np.ndarray:
    if bias is None:
        return np.zeros((t["M0"].shape[0], 1))
    return np.asarray(bias, dtype=np.float64)[:t["M0"].shape[0], None]


def reference(t: dict, bias=None) -> np.ndarray:
    return t["ref0"] + _bias64(t, bias)


def gamma_pair(cin: int, ksplit: int, has_bias: bool) -> int:
    return cin + 2 + (ksplit - 1) + int(has_bias)


def gamma_six(cin: int, ksplit: int, has_bias: bool) -> int:
    return 6 * cin + (ksplit - 1) + int(has_bias)


def bound_pair(t: dict, bias, ksplit: int) -> np.ndarray:
    M = np.abs(_bias64(t, bias)) + t["M0"]
    return t["split"] + gamma_pair(t["cin"], ksplit, bias is not None) * 2.0 ** -24 * M


def bound_six(t: dict, bias, ksplit: int) -> np.ndarray:
    M = np.abs(_bias64(t, bias)) + t["M0"]
    g = gamma_six(t["cin"], ksplit, bias is not None)
    return (2.0 ** -23 + 2.0 ** -32) * t["M0"] + g * 2.0 ** -24 * (1 + 2.0 ** -6) * M + g * 2.0 ** -149


def fraction(got: np.ndarray, ref: np.ndarray, bound: np.ndarray) -> float:
    """The largest |got - ref| / bound; inf for a non-finite element or an error
    above a zero bound."""
    err = np.abs(got.astype(np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        use = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    use = np.where(np.isfinite(got), use, np.inf)
    return float(use.max()) if use.size else 0.0


# --------------------------------------------------------------------------- emulation
def _pad(a: np.ndarray, axis: int, n: int, repeat_last: bool) -> np.ndarray:
    if n == 0:
        return a
    last = np.take(a, [-1], axis=axis)
    fill = np.repeat(last if repeat_last else np.zeros_like(last), n, axis=axis)
    return np.concatenate([a, fill], axis=axis)


def split_f16(v: np.ndarray, flush: bool = False):
    """Mirrors ``dxr::split8_f16`` (csrc/mfma_operands.h): (hi, lo) as float32
    values of float16 roundings."""
    with np.errstate(over="ignore", invalid="ignore"):
        hi = v.astype(np.float16).astype(F32)
        lo = ((v - hi) * F32(2048)).astype(np.float16).astype(F32)
    if flush:
        hi, lo = (np.where(np.abs(p) < F32(F16_MIN_NORMAL), F32(0), p) for p in (hi, lo))
    return hi, lo


def _bf16_rne(v: np.ndarray) -> np.ndarray:
    u = v.astype(F32).view(np.uint32)
    r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000))
    return r.view(F32)


def split_bf16(v: np.ndarray):
    """Mirrors ``dxr::split8_bf16<GUARD_INF_AND_RANGE>`` (csrc/mfma_operands.h) for
    finite |v| below bf16's largest finite value."""
    hi = _bf16_rne(v)
    r1 = v - hi
    mid = _bf16_rne(r1)
    lo = ((r1 - mid).view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)
    return hi, mid, lo


def _steps(nks: int, ksplit: int):
    return [(h * nks // ksplit, (h + 1) * nks // ksplit) for h in range(ksplit)]


def _accumulate(acc, a, b, k0):
    """One MFMA: the 16 channel products of step k0, each exact, added in float32."""
    for c in range(16 * k0, 16 * k0 + 16):
        acc += a[:, c, None] * b[None, c, :]
    return acc


def gemm_pair(w, x, ksplit: int, flaw=None) -> np.ndarray:
    """The f16-pair GEMM before the bias, float32 [cout, Q]."""
    cin = w.shape[1]
    n = cin_pad(cin) - cin
    w, x = _pad(w, 1, n, flaw == "unpadded"), _pad(x, 0, n, flaw == "unpadded")
    wh, wl = split_f16(w, flaw == "flush")
    xh, xl = split_f16(x, flaw == "flush")
    total = None
    with np.errstate(over="ignore", invalid="ignore"):
        for kbeg, kend in _steps(w.shape[1] // 16, ksplit):
            acc = np.zeros((w.shape[0], x.shape[1]), dtype=F32)
            acc2 = np.zeros_like(acc)
            for ks in range(kbeg, kend):
                _accumulate(acc2, wl, xh, ks)
                if flaw != "drop":
                    _accumulate(acc2, wh, xl, ks)
                _accumulate(acc, wh, xh, ks)
            scale = 2.0 ** -10 if flaw == "scale" else 2.0 ** -11
            acc = (acc2.astype(np.float64) * scale + acc.astype(np.float64)).astype(F32)   # fmaf
            total = acc if total is None else total + acc
    return total


def gemm_six(w, x, ksplit: int) -> np.ndarray:
    """The three-way bf16 GEMM before the bias, float32 [cout, Q]."""
    cin = w.shape[1]
    n = cin_pad(cin) - cin
    wh, wm, wl = split_bf16(_pad(w, 1, n, False))
    xh, xm, xl = split_bf16(_pad(x, 0, n, False))
    total = None
    for kbeg, kend in _steps(wh.shape[1] // 16, ksplit):
        acc = np.zeros((w.shape[0], x.shape[1]), dtype=F32)
        for ks in range(kbeg, kend):
            for a, b in ((wm, xm), (wl, xh), (wh, xl), (wm, xh), (wh, xm), (wh, xh)):
                _accumulate(acc, a, b, ks)
        total = acc if total is None else total + acc
    return total


def _finish(acc, bias):
    return acc if bias is None else acc + np.asarray(bias, dtype=F32)[:acc.shape[0], None]


def emulate_six(w, x, bias=None, ksplit: int = 2) -> np.ndarray:
    return _finish(gemm_six(w, x, ksplit), bias)


def emulate(w, x, bias=None, ksplit: int = 2, flaw=None):
    """The kernel's arithmetic for one batch item (``x`` [cin, Q]): the pair GEMM,
    and for every workgroup of 32 queries with a non-finite sum the bf16 GEMM
    instead.  Returns (out float32 [cout, Q], fell_back bool [workgroups]).
    Flaws: ``flush`` (f16 subnormal parts read as zero), ``drop`` (no hi_w lo_x
    product), ``scale`` (acc2 times 2^-10), ``unpadded`` (both operands read the
    last real channel in the padding), ``no_fallback``."""
    if flaw is not None and flaw not in FLAWS:
        raise ValueError(flaw)
    acc = gemm_pair(w, x, ksplit, flaw)
    starts = range(0, x.shape[1], QB)
    fell = np.array([not np.isfinite(acc[:, s:s + QB]).all() for s in starts])
    if flaw != "no_fallback":
        for s, f in zip(starts, fell):
            if f:
                acc[:, s:s + QB] = gemm_six(w, x[:, s:s + QB], ksplit)
    return _finish(acc, bias), fell
