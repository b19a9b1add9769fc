"""Helpers of the lookup path and the warm start (reference core/utils/utils.py:26-54, 74-77)."""
from __future__ import annotations

import torch

from . import _native

__all__ = ["coords_grid", "forward_interpolate"]


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
