"""Numpy float64 oracle of the convex 8x upsampling (reference core/raft.py:87-98),
forward and backward, with the magnitude sums the GPU tests' tolerances scale by.

Test infrastructure only.  tests/test_upsample_cpu.py pins it against
``e2e_flow.upsample_flow`` and torch's autograd in float64.

Index convention: fine pixel (8h+i, 8w+j) uses x_k = mask[n, 64k + 8i + j, h, w];
tap k points at coarse pixel (h + k//3 - 1, w + k%3 - 1); outside the map f = 0.
"""
from __future__ import annotations

import numpy as np


def taps(f: np.ndarray) -> np.ndarray:
    """[N, C, H, W] -> [N, C, 9, H, W]: the zero-padded 3x3 neighbourhood, tap-major."""
    N, C, H, W = f.shape
    pad = np.zeros((N, C, H + 2, W + 2), dtype=f.dtype)
    pad[:, :, 1:-1, 1:-1] = f
    return np.stack([pad[:, :, k // 3:k // 3 + H, k % 3:k % 3 + W] for k in range(9)], axis=2)


def taps_adjoint(t: np.ndarray) -> np.ndarray:
    """[N, C, 9, H, W] -> [N, C, H, W]: every T[k, h, w] added where tap k of (h, w) points."""
    N, C, _, H, W = t.shape
    pad = np.zeros((N, C, H + 2, W + 2), dtype=t.dtype)
    for k in range(9):
        pad[:, :, k // 3:k // 3 + H, k % 3:k % 3 + W] += t[:, :, k]
    return pad[:, :, 1:-1, 1:-1]


def weights(mask: np.ndarray) -> np.ndarray:
    """[N, 576, H, W] -> softmax over the taps, [N, 9, 8, 8, H, W] (k, i, j)."""
    N, _, H, W = mask.shape
    x = np.asarray(mask, dtype=np.float64).reshape(N, 9, 8, 8, H, W)
    with np.errstate(invalid="ignore"):
        e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def _fine(v: np.ndarray) -> np.ndarray:
    """[N, C, 8(i), 8(j), H, W] -> [N, C, 8H, 8W]."""
    N, C, _, _, H, W = v.shape
    return v.transpose(0, 1, 4, 2, 5, 3).reshape(N, C, 8 * H, 8 * W)


def _cells(g: np.ndarray) -> np.ndarray:
    """[N, C, 8H, 8W] -> [N, C, 8(i), 8(j), H, W]."""
    N, C, H8, W8 = g.shape
    return g.reshape(N, C, H8 // 8, 8, W8 // 8, 8).transpose(0, 1, 3, 5, 2, 4)


def forward(mask, flow):
    """(out, scale): out [N, 2, 8H, 8W] and scale = sum_k w_k |8 f_{c,k}| per output."""
    w = weights(mask)
    f8 = taps(8.0 * np.asarray(flow, dtype=np.float64))
    out = np.einsum("nkijhw,nckhw->ncijhw", w, f8)
    scale = np.einsum("nkijhw,nckhw->ncijhw", w, np.abs(f8))
    return _fine(out), _fine(scale)


def backward(mask, flow, grad_out):
    """(grad_mask, grad_flow, scale_mask, scale_flow) for out = forward(mask, flow).

    scale_mask = w_k (A_k + sum_m w_m A_m) with A_k = sum_c |g_c| |8 f_{c,k}|;
    scale_flow = 8 sum w_k |g_c| over the index set of grad_flow."""
    N, _, H, W = mask.shape
    w = weights(mask)
    f8 = taps(8.0 * np.asarray(flow, dtype=np.float64))
    g = _cells(np.asarray(grad_out, dtype=np.float64))
    a = np.einsum("ncijhw,nckhw->nkijhw", g, f8)
    A = np.einsum("ncijhw,nckhw->nkijhw", np.abs(g), np.abs(f8))
    grad_mask = w * (a - (w * a).sum(axis=1, keepdims=True))
    scale_mask = w * (A + (w * A).sum(axis=1, keepdims=True))
    grad_flow = 8.0 * taps_adjoint(np.einsum("nkijhw,ncijhw->nckhw", w, g))
    scale_flow = 8.0 * taps_adjoint(np.einsum("nkijhw,ncijhw->nckhw", w, np.abs(g)))
    return (grad_mask.reshape(N, 576, H, W), grad_flow, scale_mask.reshape(N, 576, H, W),
            scale_flow)
