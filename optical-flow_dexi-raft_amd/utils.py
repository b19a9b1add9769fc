"""Helpers of the lookup path, the warm start, the upsampling and the training
loss (reference core/utils/utils.py:26-54, 74-77; core/raft.py:87-98;
train.py:48-73)."""
from __future__ import annotations

import ctypes

import torch

from . import _native

__all__ = ["coords_grid", "forward_interpolate", "upsample_flow", "sequence_loss", "flow_metrics"]


def coords_grid(batch: int, ht: int, wd: int, device=None) -> torch.Tensor:
    """``[batch, 2, ht, wd]`` float32 grid; channel 0 = x (column), 1 = y (row).

    Same values as the reference's ``coords_grid``; ``device`` lets callers build
    it directly on the GPU instead of the reference's host grid + copy
    (core/raft.py:81-82).
    """
    ys, xs = torch.meshgrid(torch.arange(ht, device=device, dtype=torch.float32),
                            torch.arange(wd, device=device, dtype=torch.float32),
                            indexing="ij")
    return torch.stack((xs, ys), dim=0)[None].repeat(batch, 1, 1, 1)


def forward_interpolate(flow: torch.Tensor) -> torch.Tensor:
    """The reference's ``forward_interpolate`` (core/utils/utils.py:26-54) on the GPU.

    ``flow``: ``[2, H, W]`` (as the reference takes it) or ``[B, 2, H, W]``, on a
    HIP device; channel 0 = dx, 1 = dy.  Returns a new contiguous float32 tensor
    of the same shape on the same device: every pixel is pushed along its flow,
    and every grid point takes the flow of the nearest pushed pixel — what the
    reference computes with a device-to-host copy and two
    ``scipy.interpolate.griddata(method='nearest')`` calls.  Here it is three HIP
    launches on torch's current stream with no host synchronisation and no copy
    to the host, so it can sit inside a captured graph.

    The rule, per item (include/dexiraft_flow.h):

    * source pixel ``i = y0*W + x0`` lands at ``x1 = float64(x0) + float64(dx[i])``,
      ``y1 = float64(y0) + float64(dy[i])`` (numpy's int64 + float32 promotion);
    * it is valid iff ``0 < x1 < W and 0 < y1 < H`` (strict, utils.py:41); NaN and
      infinite flows fail the comparisons and drop out;
    * grid point ``(gx, gy)`` takes the ``(dx, dy)`` of the valid source with the
      smallest ``d2 = (gx - x1)**2 + (gy - y1)**2`` in float64, each operation
      rounded on its own (no fused multiply-add);
    * among equal ``d2`` the lowest ``i`` wins (scipy leaves ties unspecified; here
      they are specified, so results are deterministic and bit-reproducible);
    * the two float32 values are copied bit for bit (``-0.0`` stays ``-0.0``);
    * an item with no valid source is all zeros — the one deliberate difference:
      the reference raises inside scipy there.

    float16 / bfloat16 inputs are widened and non-contiguous ones made contiguous
    first (the reference sees float32 after ``.float()``).  Like the reference,
    which detaches, this has no gradient: an input that requires grad under grad
    mode raises ``NotImplementedError`` (detach it, or call under ``no_grad``).
    Host tensors raise ``RuntimeError`` (there is no CPU path), other ranks or a
    channel count other than 2 ``ValueError``.  The workspace comes from torch's
    caching allocator.
    """
    if not isinstance(flow, torch.Tensor):
        raise TypeError(f"flow must be a torch.Tensor, got {type(flow).__name__}")
    if flow.dim() not in (3, 4) or flow.shape[-3] != 2:
        raise ValueError(f"flow must be [2, H, W] or [B, 2, H, W], got {tuple(flow.shape)}")
    if flow.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("forward_interpolate has no gradient (the reference detaches): "
                                  "detach the flow or call under torch.no_grad()")
    if not flow.is_cuda:
        raise RuntimeError("forward_interpolate: flow must be on a HIP device (no CPU path)")
    if flow.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError(f"flow must be float32, float16 or bfloat16, got {flow.dtype}")
    lib = _native.load()
    x = flow.detach().float().contiguous()
    H, W = int(x.shape[-2]), int(x.shape[-1])
    B = int(x.shape[0]) if x.dim() == 4 else 1
    with torch.cuda.device(x.device):
        out = torch.empty_like(x)
        nbytes = lib.dxf_forward_interpolate_workspace_bytes(B, H, W)
        if nbytes < 0:
            raise RuntimeError(f"forward_interpolate: unsupported geometry B={B}, H={H}, W={W} "
                               "(B <= 65535, 1 <= H*W <= 2**22)")
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x.device)
        _native.check(lib.dxf_forward_interpolate(_native.ptr(x), B, H, W, _native.ptr(out),
                                                  _native.ptr(ws), nbytes, _native.stream_of(x)),
                      "dxf_forward_interpolate")
    return out


_MASK_DTYPES = {torch.float32: _native.DXU_MASK_F32, torch.float16: _native.DXU_MASK_F16,
                torch.bfloat16: _native.DXU_MASK_BF16}


class _ConvexUpsample(torch.autograd.Function):
    """flow: [N, 2, H, W] float32, mask: [N, 576, H, W] of a supported dtype, both
    contiguous and on one HIP device.  Saves its two inputs and nothing else."""

    @staticmethod
    def forward(ctx, flow, mask):
        ctx.save_for_backward(flow, mask)
        lib = _native.load()
        N, _, H, W = flow.shape
        with torch.cuda.device(flow.device):
            out = torch.empty((N, 2, 8 * H, 8 * W), dtype=torch.float32, device=flow.device)
            _native.check(lib.dxu_convex_upsample(_native.ptr(mask), _MASK_DTYPES[mask.dtype],
                                                  _native.ptr(flow), N, H, W, _native.ptr(out),
                                                  _native.stream_of(flow)),
                          "dxu_convex_upsample")
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        flow, mask = ctx.saved_tensors
        need_flow, need_mask = ctx.needs_input_grad
        if not (need_flow or need_mask):
            return None, None
        lib = _native.load()
        N, _, H, W = flow.shape
        g = grad_out.float().contiguous()
        with torch.cuda.device(flow.device):
            grad_flow = torch.empty_like(flow) if need_flow else None
            grad_mask = torch.empty_like(mask) if need_mask else None
            ws, nbytes = None, 0
            if need_flow:
                nbytes = lib.dxu_convex_upsample_backward_workspace_bytes(N, H, W)
                ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=flow.device)
            _native.check(lib.dxu_convex_upsample_backward(
                _native.ptr(g), _native.ptr(mask), _MASK_DTYPES[mask.dtype], _native.ptr(flow),
                N, H, W, _native.ptr(grad_mask), _native.ptr(grad_flow), _native.ptr(ws), nbytes,
                _native.stream_of(flow)), "dxu_convex_upsample_backward")
        return grad_flow, grad_mask


def upsample_flow(flow: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """The reference's ``RAFT.upsample_flow`` (core/raft.py:87-98), fused, on the GPU.

    ``flow``: ``[N, 2, H, W]``, ``mask``: ``[N, 576, H, W]`` (the update block's mask
    head), on one HIP device.  Returns the ``[N, 2, 8H, 8W]`` float32 flow: fine
    pixel ``(8h+i, 8w+j)`` is the convex combination of the 3x3 neighbourhood of
    ``8 * flow`` around ``(h, w)`` (zeros outside the map) with the weights
    ``softmax_k mask[n, 64k + 8i + j, h, w]``, ``k = 0..8``.  One HIP launch that
    reads the mask once and writes the output once, where the reference runs
    ``view -> softmax -> unfold -> multiply -> sum -> permute -> reshape``.

    Differentiable in both arguments.  The backward recomputes the softmax from
    the two inputs, which are all that is saved (the torch chain keeps the softmax
    output of every iteration alive), honours ``needs_input_grad``, is
    deterministic (no atomics) and takes two launches; its workspace and the
    outputs come from torch's caching allocator, everything runs on torch's
    current stream without a synchronisation, so forward and backward can sit
    inside a captured graph.  Double backward is not supported and raises.

    The mask may be float32, float16 or bfloat16 and is read in place; all
    arithmetic is float32.  This is the one difference from the reference: with a
    16-bit mask its softmax rounds the weights to 16 bits, here the result is the
    float32 computation on ``mask.float()``.  ``grad_mask`` has the mask's dtype
    (the float32 value rounded once).  A float16 / bfloat16 ``flow`` is widened
    first.  Non-contiguous inputs, a channels-last mask included, are made
    contiguous by a copy.

    Host tensors raise ``RuntimeError`` (there is no CPU path); wrong ranks, a
    channel count other than 2 / 576, mismatched ``N``/``H``/``W`` or tensors on
    different devices ``ValueError``; other dtypes ``TypeError``.
    """
    for name, t in (("flow", flow), ("mask", mask)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    if flow.dim() != 4 or flow.shape[1] != 2:
        raise ValueError(f"flow must be [N, 2, H, W], got {tuple(flow.shape)}")
    if mask.dim() != 4 or mask.shape[1] != 576:
        raise ValueError(f"mask must be [N, 576, H, W], got {tuple(mask.shape)}")
    if (mask.shape[0], *mask.shape[2:]) != (flow.shape[0], *flow.shape[2:]):
        raise ValueError(f"flow {tuple(flow.shape)} and mask {tuple(mask.shape)} differ in N, H or W")
    if flow.device != mask.device:
        raise ValueError(f"flow is on {flow.device}, mask on {mask.device}")
    if mask.dtype not in _MASK_DTYPES:
        raise TypeError(f"mask must be float32, float16 or bfloat16, got {mask.dtype}")
    if flow.dtype not in _MASK_DTYPES:
        raise TypeError(f"flow must be float32, float16 or bfloat16, got {flow.dtype}")
    if not flow.is_cuda:
        raise RuntimeError("upsample_flow: flow and mask must be on a HIP device (no CPU path)")
    N, _, H, W = flow.shape
    if N > 65535 or H < 1 or W < 1 or H * W > 2 ** 22:
        raise ValueError(f"upsample_flow: unsupported geometry N={N}, H={H}, W={W} "
                         "(N <= 65535, 1 <= H*W <= 2**22)")
    return _ConvexUpsample.apply(flow.float().contiguous(), mask.contiguous())


def _pointer_array(tensors):
    """Host array of device pointers (null for None), as the dxl_ entry points take it."""
    return (ctypes.c_void_p * len(tensors))(*[_native.ptr(t) for t in tensors])


def _loss_forward(preds, flow_gt, valid, gamma, max_flow, want_loss):
    """dxl_sequence_loss on contiguous float32 tensors of one HIP device: (loss,
    terms, stats), the first two None unless ``want_loss``."""
    lib = _native.load()
    B, _, H, W = flow_gt.shape
    P, dev = len(preds), flow_gt.device
    with torch.cuda.device(dev):
        loss = torch.empty((), dtype=torch.float32, device=dev) if want_loss else None
        terms = torch.empty(P, dtype=torch.float32, device=dev) if want_loss else None
        stats = torch.empty(6, dtype=torch.float64, device=dev)
        nbytes = lib.dxl_sequence_loss_workspace_bytes(P, B, H, W)
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        _native.check(lib.dxl_sequence_loss(
            _pointer_array(preds), P, _native.ptr(flow_gt), _native.ptr(valid), B, H, W, gamma,
            max_flow, _native.ptr(loss), _native.ptr(terms), _native.ptr(stats), _native.ptr(ws),
            nbytes, _native.stream_of(flow_gt)), "dxl_sequence_loss")
    return loss, terms, stats


class _SequenceLoss(torch.autograd.Function):
    """flow_gt: [B, 2, H, W], valid: [B, H, W] or None, preds: P tensors like flow_gt;
    all float32, contiguous, on one HIP device.  Saves references to its inputs and
    nothing else; returns (loss, terms, stats), differentiable in the predictions
    through ``loss`` only."""

    @staticmethod
    def forward(ctx, flow_gt, valid, gamma, max_flow, *preds):
        ctx.save_for_backward(flow_gt, valid, *preds)
        ctx.gamma, ctx.max_flow = gamma, max_flow
        loss, terms, stats = _loss_forward(preds, flow_gt, valid, gamma, max_flow, True)
        ctx.mark_non_differentiable(terms, stats)
        return loss, terms, stats

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss, _grad_terms, _grad_stats):
        flow_gt, valid, *preds = ctx.saved_tensors
        need = ctx.needs_input_grad[4:]
        if not any(need):
            return (None,) * (4 + len(preds))
        lib = _native.load()
        B, _, H, W = flow_gt.shape
        with torch.cuda.device(flow_gt.device):
            g = grad_loss.float().contiguous()
            grads = [torch.empty_like(p) if n else None for p, n in zip(preds, need)]
            _native.check(lib.dxl_sequence_loss_backward(
                _native.ptr(g), _pointer_array(preds), _pointer_array(grads), len(preds),
                _native.ptr(flow_gt), _native.ptr(valid), B, H, W, ctx.gamma, ctx.max_flow,
                _native.stream_of(flow_gt)), "dxl_sequence_loss_backward")
        return (None, None, None, None, *grads)


def _check_loss_inputs(what, preds, flow_gt, valid):
    for name, t in (*((f"flow_preds[{i}]", p) for i, p in enumerate(preds)), ("flow_gt", flow_gt),
                    *((("valid", valid),) if valid is not None else ())):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    if not 1 <= len(preds) <= 32:
        raise ValueError(f"{what}: 1 to 32 predictions, got {len(preds)}")
    if flow_gt.dim() != 4 or flow_gt.shape[1] != 2:
        raise ValueError(f"flow_gt must be [B, 2, H, W], got {tuple(flow_gt.shape)}")
    B, _, H, W = flow_gt.shape
    for i, p in enumerate(preds):
        if p.shape != flow_gt.shape:
            raise ValueError(f"flow_preds[{i}] is {tuple(p.shape)}, flow_gt {tuple(flow_gt.shape)}")
    if valid is not None and tuple(valid.shape) != (B, H, W):
        raise ValueError(f"valid must be [B, H, W] = {(B, H, W)}, got {tuple(valid.shape)}")
    if B < 1 or H < 1 or W < 1 or B * H * W > 2 ** 31:
        raise ValueError(f"{what}: unsupported geometry B={B}, H={H}, W={W} "
                         "(B, H, W >= 1, B*H*W <= 2**31)")
    for i, p in enumerate((flow_gt, *preds)):
        if p.device != flow_gt.device or (valid is not None and valid.device != flow_gt.device):
            raise ValueError(f"{what}: tensors on different devices")
        if not p.is_floating_point():
            raise TypeError(f"{what}: flows must be floating point, got {p.dtype}")
    if not flow_gt.is_cuda:
        raise RuntimeError(f"{what}: the tensors must be on a HIP device (no CPU path)")


def sequence_loss(flow_preds, flow_gt, valid, gamma=0.8, max_flow=400.0, *, sync_metrics=True):
    """The reference's ``sequence_loss`` (train.py:48-73), fused, on the GPU.

    ``flow_preds``: 1 to 32 predictions ``[B, 2, H, W]``, ``flow_gt``: ``[B, 2, H, W]``,
    ``valid``: ``[B, H, W]`` (or ``None``: all valid), on one HIP device.  Returns
    ``(loss, metrics)`` as the reference does.  With ``M = 2*B*H*W``::

        v      = (valid >= 0.5) & (sqrt(gx*gx + gy*gy) < max_flow)
        term_i = (1/M) * sum v * |flow_preds[i] - flow_gt|
        loss   = sum_i gamma**(P-1-i) * term_i

    ``loss`` is a 0-dim float32 tensor, differentiable in every prediction that
    requires grad (not in ``flow_gt`` or ``valid``): every gradient element is
    ``+q_i``, ``-q_i`` or ``0`` with ``q_i = float32(gamma**(P-1-i) / M) * grad_loss``.
    ``metrics`` is ``{'epe', '1px', '3px', '5px'}`` as Python floats, from the last
    prediction over the pixels ``v`` selects, read with one device-to-host copy of
    six numbers; with no pixel selected they are NaN, like the reference's empty
    mean.  With ``sync_metrics=False`` nothing is copied or synchronised and
    ``metrics`` is ``{'stats': float64[6], 'terms': float32[P]}`` on the device
    (``stats`` as ``flow_metrics`` returns it), so the call can sit inside a
    captured graph.

    The forward is two HIP launches that read every prediction once, where the
    reference runs six torch ops per prediction and nine reductions; the backward
    is one launch that recomputes ``v`` and the signs from the inputs, which are
    all that is saved (by reference).  No atomics: both are deterministic.  Sums
    are float64 above 16 float32 additions per thread and a wave-wide tree.  As in
    the reference, a non-finite prediction makes the loss NaN even at an invalid
    pixel.  Double backward is not supported and raises.

    Predictions of other floating dtypes are widened with ``.float()`` (autograd
    carries the conversion), ``valid`` of any dtype is converted with ``.float()``,
    non-contiguous inputs are copied.  Host tensors raise ``RuntimeError`` (there
    is no CPU path); wrong ranks or shapes, an empty batch, more than 32
    predictions or tensors on different devices ``ValueError``.
    """
    preds = list(flow_preds)
    gamma, max_flow = float(gamma), float(max_flow)
    if not gamma >= 0.0 or max_flow != max_flow:
        raise ValueError(f"sequence_loss: gamma must be >= 0 and max_flow not NaN, got {gamma}, "
                         f"{max_flow}")
    _check_loss_inputs("sequence_loss", preds, flow_gt, valid)
    loss, terms, stats = _SequenceLoss.apply(
        flow_gt.detach().float().contiguous(),
        None if valid is None else valid.detach().float().contiguous(), gamma, max_flow,
        *(p.float().contiguous() for p in preds))
    if not sync_metrics:
        return loss, {"stats": stats, "terms": terms}
    n, epe, px1, px3, px5, _ = stats.tolist()
    nan = float("nan")
    return loss, {"epe": epe / n if n else nan, "1px": px1 / n if n else nan,
                  "3px": px3 / n if n else nan, "5px": px5 / n if n else nan}


def flow_metrics(flow_pr, flow_gt, valid=None, max_flow=float("inf")):
    """End-point-error statistics of one flow on the GPU (evaluate.py:93, 121-128,
    154-169 without the copy of the flow to the host).

    ``flow_pr``, ``flow_gt``: ``[B, 2, H, W]`` (or ``[2, H, W]``), ``valid``:
    ``[B, H, W]`` (``[H, W]``) or ``None``.  Returns the float64 tensor
    ``[count, sum epe, #(epe < 1), #(epe < 3), #(epe < 5), #(epe > 3 and epe/mag > 0.05)]``
    on the device, over the pixels with ``valid >= 0.5`` and ``mag < max_flow``,
    ``epe = |flow_pr - flow_gt|``, ``mag = |flow_gt|`` (float32 per pixel, exact
    counts): mean EPE is ``s[1] / s[0]``, the pixel fractions ``s[2:5] / s[0]``,
    KITTI's F1 ``100 * s[5] / s[0]``.  The forward of ``sequence_loss`` with one
    prediction; no gradient, no synchronisation.
    """
    if isinstance(flow_pr, torch.Tensor) and flow_pr.dim() == 3:
        flow_pr, flow_gt = flow_pr[None], flow_gt[None]
        valid = None if valid is None else valid[None]
    _check_loss_inputs("flow_metrics", [flow_pr], flow_gt, valid)
    max_flow = float(max_flow)
    if max_flow != max_flow:
        raise ValueError("flow_metrics: max_flow must not be NaN")
    with torch.no_grad():
        return _loss_forward([flow_pr.float().contiguous()], flow_gt.float().contiguous(),
                             None if valid is None else valid.float().contiguous(), 1.0,
                             max_flow, False)[2]
