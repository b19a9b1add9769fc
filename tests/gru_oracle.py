"""float64 oracle of the fused SepConvGRU forward (include/dexiraft_gru.h), a
restatement of the reference's core/update.py:45-60 with the stated roundings.

With c the compute dtype (``"f16"``, ``"bf16"``, or ``None`` for no rounding at
all) and rne_c rounding to nearest even into c, for axis 0 (taps along W), then
axis 1 (taps along H):

  1. hc = rne_c(h), xc = rne_c(x), Wc = rne_c(W); biases as they are
  2. Pz, Pr = b + sum_t sum_ci Wc[co, ci, t] * [hc | xc][ci, p + t - 2], zero past
     the ends of the row / the image column
  3. z = sigmoid(Pz), r = sigmoid(Pr); rh = rne_c(r * h)
  4. Pq as 2. on [rh | xc]; q = tanh(Pq); h <- (1 - z) h + z q

Everything is float64 on NCHW arrays; every stage also returns
S = |b| + sum |Wc| |a| of each pre-activation, the scale of its float32
accumulation error.  ``case()`` makes the seeded inputs the goldens
(tests/golden/make_gru_golden.py) and the GPU tests share.
"""
from __future__ import annotations

import numpy as np

import datagen as dg

NAMES = ("convz1", "convr1", "convq1", "convz2", "convr2", "convq2")
P_BITS = {"f16": 11, "bf16": 8}     # significand bits of c: rne_c is within 2^-p relative


def rne(a, c):
    """float64 -> nearest-even c, as float64 (None: the identity).  bfloat16 is
    rounded straight from the float64 bits (no float32 step in between); values are
    assumed inside c's normal range for bfloat16, float16 goes through numpy."""
    a = np.asarray(a, dtype=np.float64)
    if c is None:
        return a
    if c == "f16":
        with np.errstate(over="ignore"):
            return a.astype(np.float16).astype(np.float64)
    if c == "bf16":
        u = a.view(np.uint64) if a.flags.c_contiguous else np.ascontiguousarray(a).view(np.uint64)
        drop = np.uint64(45)      # float64 keeps 52 fraction bits, bfloat16 7
        bias = ((u >> drop) & np.uint64(1)) + np.uint64((1 << 44) - 1)
        with np.errstate(over="ignore"):
            v = (u + bias) & ~np.uint64((1 << 45) - 1)
        return v.view(np.float64).reshape(a.shape)
    raise ValueError(c)


def sigmoid(p):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-p))


def w3(w):
    """[Ch, C, 1, 5] or [Ch, C, 5, 1] -> [Ch, C, 5] float64."""
    w = np.asarray(w, dtype=np.float64)
    return w.reshape(w.shape[0], w.shape[1], 5)


def conv5(a, w, b, axis):
    """P = b + the 5-tap convolution of a [N, C, H, W] with w [Co, C, 5] along W
    (axis 0) or H (axis 1), zero padded; and S = |b| + sum |w| |a|."""
    N, C, H, W = a.shape
    pad = ((0, 0), (0, 0), (0, 0), (2, 2)) if axis == 0 else ((0, 0), (0, 0), (2, 2), (0, 0))
    ap = np.pad(a, pad)
    P = np.broadcast_to(b[None, :, None, None], (N, w.shape[0], H, W)).astype(np.float64)
    S = np.abs(P)
    for t in range(5):
        sl = ap[:, :, :, t:t + W] if axis == 0 else ap[:, :, t:t + H, :]
        P = P + np.einsum("oc,nchw->nohw", w[:, :, t], sl)
        S = S + np.einsum("oc,nchw->nohw", np.abs(w[:, :, t]), np.abs(sl))
    return P, S


def stage_zr(hc, xc, h, wz, bz, wr, br, axis, c):
    """Steps 2 and 3 on given operands (hc, xc already in c; h the float32 state)."""
    a = np.concatenate([hc, xc], axis=1)
    Pz, Sz = conv5(a, wz, bz, axis)
    Pr, Sr = conv5(a, wr, br, axis)
    z, r = sigmoid(Pz), sigmoid(Pr)
    return {"Pz": Pz, "Sz": Sz, "Pr": Pr, "Sr": Sr, "z": z, "r": r, "rh_exact": r * h,
            "rh": rne(r * h, c)}


def stage_qh(rh, xc, z, h, wq, bq, axis):
    """Step 4 on given operands."""
    Pq, Sq = conv5(np.concatenate([rh, xc], axis=1), wq, bq, axis)
    q = np.tanh(Pq)
    return {"Pq": Pq, "Sq": Sq, "q": q, "h": (1.0 - z) * h + z * q}


def forward(h, x, weights, c):
    """The whole definition; ``weights`` maps convz1.weight ... convq2.bias.
    Returns the final h (float64, NCHW, not yet cast to the output dtype)."""
    h = np.asarray(h, dtype=np.float64)
    xc = rne(x, c)
    for axis in range(2):
        wz, wr, wq = (rne(w3(weights[f"{n}.weight"]), c) for n in NAMES[3 * axis:3 * axis + 3])
        bz, br, bq = (np.asarray(weights[f"{n}.bias"], dtype=np.float64)
                      for n in NAMES[3 * axis:3 * axis + 3])
        zr = stage_zr(rne(h, c), xc, h, wz, bz, wr, br, axis, c)
        h = stage_qh(zr["rh"], xc, zr["z"], h, wq, bq, axis)["h"]
    return h


def case(seed: int, N: int, H: int, W: int, Ch: int, Cx: int, h_floor: float = 0.0):
    """Seeded float32 inputs: h = tanh(N(0, 1)) (a GRU state lies in (-1, 1)),
    x ~ N(0, 1), the six weights normal with standard deviation 1 / sqrt(K),
    K = 5 (Ch + Cx) (pre-activations of unit scale: the gates are not saturated),
    all different and asymmetric in taps and channels, biases of deviation 0.5.
    With ``h_floor`` the state is pushed away from zero, sign kept:
    |h| = h_floor + (1 - h_floor) |tanh|, so that |h| >= h_floor."""
    C, K = Ch + Cx, 5 * (Ch + Cx)
    t = np.tanh(dg.normal(seed, N * Ch * H * W))
    if h_floor:
        t = np.where(t < 0, -1.0, 1.0) * (h_floor + (1.0 - h_floor) * np.abs(t))
    h = t.reshape(N, Ch, H, W).astype(np.float32)
    x = dg.normal(seed + 1, N * Cx * H * W).reshape(N, Cx, H, W).astype(np.float32)
    weights = {}
    for i, name in enumerate(NAMES):
        shape = (Ch, C, 1, 5) if i < 3 else (Ch, C, 5, 1)
        w = dg.normal(seed + 10 + 2 * i, Ch * K) / np.sqrt(K)
        weights[f"{name}.weight"] = w.reshape(shape).astype(np.float32)
        weights[f"{name}.bias"] = (0.5 * dg.normal(seed + 11 + 2 * i, Ch)).astype(np.float32)
    return h, x, weights
