"""Numpy oracle of the sequence loss and the flow statistics
(include/dexiraft_loss.h), written from the definition, in two forms.

Inputs: ``preds`` a list of P float32 arrays [B, 2, H, W], ``gt`` the same shape,
``valid`` [B, H, W] float32 or None (all valid).  With M = 2*B*H*W::

    mag    = sqrt(gx*gx + gy*gy)
    v      = (valid >= 0.5) & (mag < max_flow)
    term_i = (1/M) * sum v * |p_i - g|
    w_i    = gamma ** (P-1-i)                       Python float (double)
    loss   = sum_i w_i * term_i
    epe    = sqrt(dx*dx + dy*dy) of the last prediction
    stats  = [count(v), sum_v epe, #(epe<1), #(epe<3), #(epe<5), #(epe>3 & epe/mag>0.05)]
    grad_i = float32(w_i / M) * grad_loss * v * sgn(p_i - g)

``sums64``: the sums (terms, loss, stats[1]) in float64, on the float32 ``v``.
``mask32`` / ``stats32`` / ``grads32``: the float32 restatement of ``v``, ``epe``,
the counts and the gradient bits: ``np.float32`` arithmetic, every operation
rounded on its own (numpy fuses nothing), square root and division correctly
rounded.  ``torch_sequence`` is the same definition as a torch op sequence, for
autograd in float64 on the CPU and for the comparison arm on the GPU.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32


def weights(P: int, gamma: float) -> list[float]:
    return [float(gamma) ** (P - 1 - i) for i in range(P)]


def mask32(gt, valid, max_flow):
    """(v [B, H, W] bool, mag [B, H, W] float32)."""
    assert gt.dtype == F32
    gx, gy = gt[:, 0], gt[:, 1]
    mag = np.sqrt(gx * gx + gy * gy)
    assert mag.dtype == F32
    v = mag < F32(max_flow)
    if valid is not None:
        assert valid.dtype == F32
        v &= valid >= F32(0.5)
    return v, mag


def sums64(preds, gt, valid, gamma, max_flow):
    """(loss, terms [P], sum_v epe) in float64."""
    v, _ = mask32(gt, valid, max_flow)
    g = gt.astype(np.float64)
    M = gt.size
    terms = np.array([(v[:, None] * np.abs(p.astype(np.float64) - g)).sum() / M for p in preds])
    loss = sum(w * t for w, t in zip(weights(len(preds), gamma), terms))
    d = preds[-1].astype(np.float64) - g
    epe = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    return float(loss), terms, float(epe[v].sum())


def epe32(pred, gt):
    assert pred.dtype == F32 and gt.dtype == F32
    dx, dy = pred[:, 0] - gt[:, 0], pred[:, 1] - gt[:, 1]
    epe = np.sqrt(dx * dx + dy * dy)
    assert epe.dtype == F32
    return epe


def stats32(pred, gt, valid, max_flow):
    """The five exact counts: [count(v), #(epe<1), #(epe<3), #(epe<5), outliers]."""
    v, mag = mask32(gt, valid, max_flow)
    epe = epe32(pred, gt)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = epe / mag
    assert ratio.dtype == F32
    out = v & (epe > F32(3)) & (ratio > F32(0.05))
    return [int(v.sum()), int((v & (epe < F32(1))).sum()), int((v & (epe < F32(3))).sum()),
            int((v & (epe < F32(5))).sum()), int(out.sum())]


def grads32(preds, gt, valid, gamma, max_flow, grad_loss=1.0):
    """The float32 gradient of every prediction, bit for bit: +q_i, -q_i or 0."""
    v, _ = mask32(gt, valid, max_flow)
    M = gt.size
    out = []
    for w, p in zip(weights(len(preds), gamma), preds):
        q = F32(w / M) * F32(grad_loss)
        assert q.dtype == F32
        d = p - gt
        sel = v[:, None]
        out.append(np.where(sel & (d > 0), q, np.where(sel & (d < 0), -q, F32(0))).astype(F32))
    return out


def grads64(preds, gt, valid, gamma, max_flow, grad_loss=1.0):
    v, _ = mask32(gt, valid, max_flow)
    M = gt.size
    g = gt.astype(np.float64)
    return [w / M * grad_loss * v[:, None] * np.sign(p.astype(np.float64) - g)
            for w, p in zip(weights(len(preds), gamma), preds)]


def torch_sequence(preds, gt, valid, gamma, max_flow):
    """The definition as torch ops, in the tensors' dtype: (loss, [count, sum epe,
    #<1, #<3, #<5]).  Differentiable in the predictions."""
    import torch
    P = len(preds)
    mag = (gt * gt).sum(dim=1).sqrt()
    v = mag < max_flow
    if valid is not None:
        v = v & (valid >= 0.5)
    loss = 0.0
    for i, p in enumerate(preds):
        loss = loss + float(gamma) ** (P - 1 - i) * (v[:, None] * (p - gt).abs()).mean()
    d = preds[-1] - gt
    epe = (d * d).sum(dim=1).sqrt()
    # selection by v as masked sums, not boolean indexing: no host synchronisation, so
    # the sequence can be captured in a graph
    stats = torch.stack([v.sum().double(), torch.where(v, epe, torch.zeros_like(epe)).double().sum(),
                         (v & (epe < 1)).sum().double(), (v & (epe < 3)).sum().double(),
                         (v & (epe < 5)).sum().double()])
    return loss, stats
