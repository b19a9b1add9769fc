"""MI355X-native drop-in for the reference ``core/corr.py``.

``CorrBlock`` and ``AlternateCorrBlock`` keep the reference constructors and
``__call__(coords)`` signatures (core/corr.py:12-91), so ``core/raft*.py`` and
``core/update.py`` run unchanged on top of them.  All arithmetic happens in the
HIP kernels of ``libdexiraft_corr.so``; the Python side only validates,
allocates (from torch's caching allocator) and launches on torch's current
stream.  There is no CPU path: host tensors raise.

Training: with float32 fmaps that require grad (under grad mode), the block is
differentiable with respect to the fmaps, as the reference is through matmul /
avg_pool2d / grid_sample (train.py:175-178).  Each lookup's backward adds its
bilinear transpose into one gradient pyramid owned by the block
(``dxr_corr_lookup_backward_multi``, a few lookups per launch); the build's
backward runs once after all of them and takes the fmap gradients as two MFMA GEMMs that fold that pyramid down
the pooling chain in their operand loads (``dxr_fmap_grads``: no [B, N, N]
volume gradient).  Shapes it does not cover (D % 32 != 0, more than 4 levels)
form dV (``dxr_pyramid_backward``) and run two torch.bmm (rocBLAS).

Differences from the reference, all loud:
  * host (CPU) tensors raise ``RuntimeError`` instead of running on the CPU;
  * coords that require grad raise ``NotImplementedError`` (the reference
    detaches them, core/raft.py:170; no grid gradient is implemented), as do
    bfloat16 or float16 fmaps that require grad and AlternateCorrBlock inputs
    that require grad (the reference's alt_cuda_corr output carries no autograd graph).

``TrainableAlternateCorrBlock`` is the on-the-fly block with fmap gradients
(O(H*W*D) memory in the backward too): same constructor and ``__call__``.
"""
from __future__ import annotations

import ctypes
import inspect
from functools import lru_cache

import numpy as np
import torch

from . import _native as nat

__all__ = ["CorrBlock", "AlternateCorrBlock", "TrainableAlternateCorrBlock"]


@lru_cache(maxsize=None)
def _sqrt_dim(dim: int) -> float:
    # torch.sqrt(torch.tensor(dim).float()) (core/corr.py:60,91): f32 IEEE sqrt.
    return float(np.sqrt(np.float32(dim), dtype=np.float32))


def _require_device(t: torch.Tensor, name: str) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    if t.device.type != "cuda":
        raise RuntimeError(
            f"{name} is on {t.device}; dexiraft_amd runs only on HIP devices (no CPU path)")


def _require_no_grad(*ts: torch.Tensor, what: str = "these inputs") -> None:
    if torch.is_grad_enabled() and any(t.requires_grad for t in ts):
        raise NotImplementedError(
            f"dexiraft_amd: no gradient is implemented for {what} (wrap the call in "
            "torch.no_grad() or detach the inputs)")


def _wants_grad(*ts: torch.Tensor) -> bool:
    return torch.is_grad_enabled() and any(t.requires_grad for t in ts)


def _volume_grads(ctx_needs, f1: torch.Tensor, f2: torch.Tensor, dv: torch.Tensor):
    """d/d fmap of corr = f1^T f2 given dV = d loss / d corr ([B, N, N], already
    divided by sqrt(D)): dF1 = F2 dV^T, dF2 = F1 dV (plain GEMMs, rocBLAS)."""
    B, D, H, W = f1.shape
    N = H * W
    df1 = df2 = None
    if ctx_needs[0]:
        df1 = torch.bmm(f2.reshape(B, D, N), dv.transpose(1, 2)).reshape(B, D, H, W)
    if ctx_needs[1]:
        df2 = torch.bmm(f1.reshape(B, D, N), dv).reshape(B, D, H, W)
    return df1, df2


class _GradState:
    """What the backward of a differentiable CorrBlock needs: its geometry and
    the gradient pyramid the lookups' backwards add into.  Held by the block
    and by the autograd nodes, it references neither the block nor the graph,
    so no reference cycle keeps the pyramid (``block._buf``) or the gradient
    pyramid alive after the step: both are freed by refcount."""

    __slots__ = ("geom", "num_levels", "radius", "device", "numel", "nslots", "grad_pyr",
                 "zero_ev", "pending", "end_hook")

    def __init__(self, geom, num_levels, radius, device, numel):
        self.geom, self.num_levels, self.radius = geom, num_levels, radius
        self.device, self.numel = device, numel
        B, _, H, W = geom
        # the lookup backwards' magnitude bound (one float per workgroup), kept
        # after the gradient pyramid in the same zero-filled buffer
        self.nslots = max(int(nat.load().dxr_lookup_backward_bound_slots(B, H, W, num_levels,
                                                                          radius)), 0)
        self.grad_pyr = None
        self.zero_ev = None   # the side-stream zero fill of grad_pyr, until a launch waits on it
        self.pending = []   # (coords, grad_out) of lookups whose backward is not applied yet
        self.end_hook = False   # an end-of-backward-pass callback is queued

    def flush(self):
        """Add the pending lookups' backwards into the gradient pyramid, in the
        order autograd delivered them, with one launch per _BW_SETS lookups
        (dxr_corr_lookup_backward_multi: bit-identical to one launch each)."""
        if not self.pending:
            return
        if self.grad_pyr is None:
            self.grad_pyr = torch.zeros(self.numel + self.nslots, dtype=torch.float32,
                                        device=self.device)
        if self.zero_ev is not None:
            torch.cuda.current_stream(self.device).wait_event(self.zero_ev)
            self.zero_ev = None
        B, D, H, W = self.geom
        n = len(self.pending)
        cs = (ctypes.c_void_p * n)(*[c.data_ptr() for c, _ in self.pending])
        gs = (ctypes.c_void_p * n)(*[g.data_ptr() for _, g in self.pending])
        lib = nat.load()
        try:
            with _Launch(self.device):
                st = lib.dxr_corr_lookup_backward_multi_bound(
                    cs, gs, n, B, H, W, self.num_levels, self.radius, self.grad_pyr.data_ptr(),
                    nat.DXR_F32, self.slots_ptr(), nat.stream_of(self.grad_pyr))
        finally:
            # never carry (coords, grad_out) entries into another flush, even if
            # the launch failed: a stale entry would be added twice
            self.pending = []
        nat.check(st, "CorrBlock lookup backward (dxr_corr_lookup_backward_multi_bound)")

    def prefill(self):
        """At a pass's first lookup backward: allocate the gradient pyramid and
        zero it on a side stream, so the fill (~270 MB at Sintel) overlaps the
        backward work that runs before the first flush instead of preceding it."""
        if self.grad_pyr is not None:
            return
        main = torch.cuda.current_stream(self.device)
        buf = torch.empty(self.numel + self.nslots, dtype=torch.float32, device=self.device)
        side = _side_stream(self.device)
        side.wait_stream(main)
        with torch.cuda.stream(side):
            buf.zero_()
        buf.record_stream(side)
        ev = torch.cuda.Event()
        ev.record(side)
        self.grad_pyr, self.zero_ev = buf, ev

    def slots_ptr(self):
        """Device address of the bound slots behind the gradient pyramid."""
        return self.grad_pyr.data_ptr() + 4 * self.numel

    def reset(self):
        """Drop pending lookups and the partial gradient pyramid (a backward pass
        that ended before the build's backward ran, e.g. an exception part-way or
        ``autograd.grad`` with inputs that stop before the build)."""
        self.pending = []
        self.grad_pyr = None
        self.zero_ev = None
        # a pass that failed elsewhere never runs its queued _end: re-arm
        # (a second queued _end is harmless, it is idempotent)
        self.end_hook = False

    def arm_end_of_pass(self):
        """Queue (once per backward pass) a callback that runs when autograd's
        pass ends: whatever the build's backward did not consume by then belongs
        to a partial pass and is dropped, so it cannot leak into the next one."""
        if self.end_hook:
            return
        self.end_hook = True

        def _end():
            self.end_hook = False
            if self.pending or self.grad_pyr is not None:
                self.reset()
        torch.autograd.Variable._execution_engine.queue_callback(_end)


_SIDE_STREAMS: dict = {}


def _side_stream(device):
    """One side stream per device for the gradient pyramid's zero fill."""
    key = torch.device(device).index
    st = _SIDE_STREAMS.get(key)
    if st is None:
        st = _SIDE_STREAMS[key] = torch.cuda.Stream(device=device)
    return st


# Lookup backwards applied per launch: their window lines stay in L2 across the
# sets; the pending grad_out tensors ([B, L*(2r+1)^2, H, W] each) live until then.
# Round 6 (profiles/r06/experiments/r6y_r6z_backward_sets.jsonl, medians of six
# alternated runs): two per launch 1.299 / 1.335 ms per Sintel training step (cloned
# inputs + mul-sum loss / persistent leaves + vdot), four 1.353 / 1.340 — the eager
# step is host-paced, and earlier flushes start the GPU sooner; peak memory alike.
_BW_SETS = 2


class _BuildGrad(torch.autograd.Function):
    """Graph node of CorrBlock.__init__: returns a scalar token every lookup
    consumes, so autograd runs this backward once, after every lookup's
    backward has added into the gradient pyramid."""

    @staticmethod
    def forward(ctx, fmap1, fmap2, gs):
        ctx.gs = gs
        ctx.save_for_backward(fmap1, fmap2)
        return fmap1.new_zeros(())

    @staticmethod
    def backward(ctx, _gtoken):
        gs = ctx.gs
        try:
            gs.flush()
        except BaseException:
            gs.reset()
            raise
        # the state is consumed here: a later pass (retain_graph) arms its own
        # end-of-pass cleanup
        gs.end_hook = False
        if gs.grad_pyr is None:
            return None, None, None
        slots = gs.slots_ptr()
        gp, gs.grad_pyr = gs.grad_pyr, None
        f1, f2 = ctx.saved_tensors
        B, D, H, W = gs.geom
        lib = nat.load()
        wsb = lib.dxr_fmap_grads_bounded_workspace_bytes(B, D, H, W, gs.num_levels)
        if wsb >= 0:   # the fused MFMA backward: no [B, N, N] dV
            need1, need2 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
            c1 = f1.contiguous() if need2 else None
            c2 = f2.contiguous() if need1 else None
            df1 = torch.empty((B, D, H, W), dtype=torch.float32, device=f1.device) if need1 else None
            df2 = torch.empty((B, D, H, W), dtype=torch.float32, device=f1.device) if need2 else None
            ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=f1.device)
            with _Launch(gs.device):
                # f16 pair GEMMs scaled by the lookups' bound (three MFMA products)
                st = lib.dxr_fmap_grads_bounded(gp.data_ptr(), nat.DXR_F32, nat.ptr(c1),
                                                nat.ptr(c2), B, D, H, W, gs.num_levels,
                                                _sqrt_dim(D), slots, gs.nslots, nat.ptr(df1),
                                                nat.ptr(df2), ws.data_ptr(), wsb,
                                                nat.stream_of(ws))
            nat.check(st, "CorrBlock backward (dxr_fmap_grads_bounded)")
            return df1, df2, None
        # D % 32 != 0 or more than 4 levels: dV, then two GEMMs
        dv = torch.empty((B, H * W, H * W), dtype=torch.float32, device=f1.device)
        with _Launch(gs.device):
            st = lib.dxr_pyramid_backward(gp.data_ptr(), nat.DXR_F32, B, H, W, gs.num_levels,
                                          _sqrt_dim(D), dv.data_ptr(), nat.stream_of(dv))
        nat.check(st, "CorrBlock backward (dxr_pyramid_backward)")
        del gp
        df1, df2 = _volume_grads(ctx.needs_input_grad, f1, f2, dv)
        return df1, df2, None


class _LookupGrad(torch.autograd.Function):
    """Graph node of CorrBlock.__call__ (differentiable in the pyramid only)."""

    @staticmethod
    def forward(ctx, token, coords, block, out_dtype=None, memory_format=None):
        ctx.gs = block._gs
        ctx.save_for_backward(coords)
        return block._lookup(coords, out_dtype, memory_format)

    @staticmethod
    def backward(ctx, gout):
        gs = ctx.gs
        (coords,) = ctx.saved_tensors
        gs.arm_end_of_pass()
        gs.prefill()
        gs.pending.append((coords, gout.contiguous().float()))
        if len(gs.pending) >= _BW_SETS:
            gs.flush()
        # no gradient for the token: autograd still runs the build's backward
        # after every lookup's (it waits on the edge, and materialises one zero)
        # without a fill per lookup and the adds that would sum them
        return None, None, None, None, None


class _VolumeGrad(torch.autograd.Function):
    """CorrBlock.corr with autograd: backward = dV / sqrt(D), two GEMMs."""

    @staticmethod
    def forward(ctx, fmap1, fmap2):
        ctx.save_for_backward(fmap1, fmap2)
        return CorrBlock._volume(fmap1, fmap2)

    @staticmethod
    def backward(ctx, gout):
        f1, f2 = ctx.saved_tensors
        B, D, H, W = f1.shape
        dv = gout.reshape(B, H * W, H * W).float() / _sqrt_dim(D)
        df1, df2 = _volume_grads(ctx.needs_input_grad, f1, f2, dv)
        return df1, df2


def _fmap_geometry(fmap1: torch.Tensor, fmap2: torch.Tensor) -> tuple[int, int, int, int]:
    _require_device(fmap1, "fmap1")
    _require_device(fmap2, "fmap2")
    if fmap1.dim() != 4 or fmap2.dim() != 4:
        raise RuntimeError(f"fmaps must be [B, D, H, W]; got {tuple(fmap1.shape)} and "
                           f"{tuple(fmap2.shape)}")
    if fmap1.shape != fmap2.shape:
        raise RuntimeError(f"fmap1 {tuple(fmap1.shape)} and fmap2 {tuple(fmap2.shape)} differ")
    if fmap1.device != fmap2.device:
        raise RuntimeError("fmap1 and fmap2 are on different devices")
    if fmap1.dtype != fmap2.dtype:
        raise RuntimeError(f"fmap dtypes differ: {fmap1.dtype} vs {fmap2.dtype}")
    B, D, H, W = (int(s) for s in fmap1.shape)
    return B, D, H, W


def _level_sizes(H: int, W: int, num_levels: int) -> list[tuple[int, int]]:
    sizes = [(H, W)]
    for _ in range(num_levels - 1):
        h, w = sizes[-1]
        if h < 2 or w < 2:
            # F.avg_pool2d raises here in the reference (core/corr.py:26).
            raise RuntimeError(
                f"pyramid level {len(sizes)} of a {H}x{W} fmap would be empty "
                f"(avg_pool2d of {h}x{w}); num_levels={num_levels} is too many")
        sizes.append((h // 2, w // 2))
    return sizes


def _channels_last(t: torch.Tensor) -> bool:
    """A channels-last (NHWC-strided) 4-D fmap that is not also NCHW-contiguous."""
    return t.is_contiguous(memory_format=torch.channels_last) and not t.is_contiguous()


def _dtype_code(t: torch.Tensor) -> int:
    """Element code of ``dxr_transpose`` (a bit-exact move: float16 goes as any
    16-bit pattern, DXR_BF16)."""
    if t.dtype == torch.float32:
        return nat.DXR_F32
    if t.dtype in (torch.bfloat16, torch.float16):
        return nat.DXR_BF16
    raise RuntimeError(f"fmaps must be float32, bfloat16 or float16, got {t.dtype}")


def _nchw(t: torch.Tensor) -> torch.Tensor:
    """NCHW-contiguous fmap (no autograd graph: callers use it only without grad).

    Channels-last fmaps (encoders emitting NHWC) go through
    one native tiled transpose (``dxr_transpose``); other layouts through
    ``.contiguous()`` (a no-op for the reference's own NCHW fmaps).
    """
    if not _channels_last(t):
        return t.contiguous()
    B, D, H, W = (int(s) for s in t.shape)
    out = torch.empty((B, D, H, W), dtype=t.dtype, device=t.device)
    with _Launch(t.device):
        st = nat.load().dxr_transpose(t.data_ptr(), out.data_ptr(), _dtype_code(t), B, H * W, D,
                                      nat.stream_of(t))
    nat.check(st, "NHWC -> NCHW fmap (dxr_transpose)")
    return out


def _nhwc(t: torch.Tensor) -> torch.Tensor:
    """``t.permute(0, 2, 3, 1).contiguous()`` (core/corr.py:82-83): a free view of a
    channels-last fmap, one native tiled transpose (``dxr_transpose``) otherwise."""
    if _channels_last(t):
        return t.permute(0, 2, 3, 1)
    t = t.contiguous()
    B, D, H, W = (int(s) for s in t.shape)
    out = torch.empty((B, H, W, D), dtype=t.dtype, device=t.device)
    with _Launch(t.device):
        st = nat.load().dxr_transpose(t.data_ptr(), out.data_ptr(), _dtype_code(t), B, D, H * W,
                                      nat.stream_of(t))
    nat.check(st, "NCHW -> NHWC fmap (dxr_transpose)")
    return out


def _pool_nhwc(t: torch.Tensor) -> torch.Tensor:
    """F.avg_pool2d(x, 2, stride=2) of a channels-last fmap held as [B, H, W, C]."""
    B, H, W, C = (int(s) for s in t.shape)
    out = torch.empty((B, H // 2, W // 2, C), dtype=t.dtype, device=t.device)
    with _Launch(t.device):
        st = nat.load().dxr_avg_pool2x2_nhwc(t.data_ptr(), out.data_ptr(), B, H, W, C,
                                             nat.stream_of(t))
    nat.check(st, "AlternateCorrBlock pooling (dxr_avg_pool2x2_nhwc)")
    return out


class _Launch:
    """Runs a native call with fmap's device current (multi-GPU processes)."""

    def __init__(self, device: torch.device):
        self.device = device
        self._ctx = None

    def __enter__(self):
        # torch._C._cuda_getDevice: torch.cuda.current_device() without its
        # lazy-init check (a block exists only on an initialised device)
        if self.device.index is not None and self.device.index != torch._C._cuda_getDevice():
            self._ctx = torch.cuda.device(self.device)
            self._ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self._ctx is not None:
            self._ctx.__exit__(*exc)
        return False


def _check_coords(coords: torch.Tensor, B: int, H: int, W: int, device: torch.device) -> torch.Tensor:
    _require_device(coords, "coords")
    if coords.dim() != 4 or tuple(coords.shape) != (B, 2, H, W):
        raise RuntimeError(f"coords must be [B, 2, H, W] = {(B, 2, H, W)}, got {tuple(coords.shape)}")
    if coords.device != device:
        raise RuntimeError(f"coords on {coords.device}, correlation block on {device}")
    if coords.dtype != torch.float32:
        coords = coords.float()
    return coords.contiguous()


_OUT_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def _out_flag(out_dtype) -> tuple[torch.dtype, int]:
    """(torch dtype of the output, flag or-ed onto pyr_dtype) of an ``out_dtype``
    argument: None / float32 take the float32 kernels, float16 / bfloat16 the
    16-bit stores (``DXR_OUT_F16`` / ``DXR_OUT_BF16``)."""
    if out_dtype is None or out_dtype == torch.float32:
        return torch.float32, 0
    if out_dtype == torch.float16:
        return torch.float16, nat.DXR_OUT_F16
    if out_dtype == torch.bfloat16:
        return torch.bfloat16, nat.DXR_OUT_BF16
    raise ValueError(f"out_dtype must be None or one of {', '.join(map(str, _OUT_DTYPES))}; "
                     f"got {out_dtype!r}")


def _layout_flag(memory_format) -> int:
    """Flag or-ed onto pyr_dtype for a ``memory_format`` argument: None and
    ``torch.contiguous_format`` keep the NCHW stores (0), ``torch.channels_last``
    selects the kernels' own channels-last stores (``DXR_OUT_NHWC``); anything
    else raises ``ValueError``."""
    if memory_format is None or memory_format is torch.contiguous_format:
        return 0
    if memory_format is torch.channels_last:
        return nat.DXR_OUT_NHWC
    raise ValueError("memory_format must be None, torch.contiguous_format or "
                     f"torch.channels_last; got {memory_format!r}")


def _pop_volume_dtype(extensions: dict):
    """The keyword-only ``volume_dtype=None`` of the alternate blocks' constructors.
    It is taken from ``**extensions`` so that the constructors' declared keyword
    defaults stay the two output options the C-ABI tests of those options pin;
    any other keyword is the ``TypeError`` a declared signature would raise."""
    volume_dtype = extensions.pop("volume_dtype", None)
    if extensions:
        raise TypeError("__init__() got an unexpected keyword argument "
                        f"{next(iter(extensions))!r}")
    return volume_dtype


def _f16_volumes(volume_dtype) -> bool:
    """Whether ``AlternateCorrBlock(..., volume_dtype=...)`` asks for float16 coarse
    volumes (``DXR_ALT_VOL_F16``): None / torch.float32 keep the float32 volumes,
    torch.float16 halves them; anything else raises ``ValueError``."""
    if volume_dtype is None:
        return False
    if not isinstance(volume_dtype, torch.dtype) or \
            volume_dtype not in (torch.float32, torch.float16):
        raise ValueError("volume_dtype must be None, torch.float32 or torch.float16; "
                         f"got {volume_dtype!r}")
    return volume_dtype == torch.float16


def _empty_out(shape, dtype, device, layout_flag: int) -> torch.Tensor:
    """The output tensor of a lookup: ``[B, C, H, W]``, channels-last strides
    when the kernel stores channels-last."""
    fmt = torch.channels_last if layout_flag else torch.contiguous_format
    return torch.empty(shape, dtype=dtype, device=device, memory_format=fmt)


_PYR_FMAP_DTYPES = (torch.float32, torch.float16)


def _f16_pyramid(fmap_dtype: torch.dtype, pyramid_dtype) -> bool:
    """Whether ``CorrBlock(..., pyramid_dtype=...)`` selects the float16 pyramid
    (``DXR_PYR_F16``) for fmaps of ``fmap_dtype``.  None keeps every input's
    default; torch.float32 names the default of float32 / float16 fmaps;
    torch.float16 selects the float16 pyramid for those fmaps.  Anything else, or
    a value that contradicts the fmap dtype (bfloat16 fmaps build a bfloat16
    pyramid), raises ``ValueError``."""
    if pyramid_dtype is None:
        return False
    if not isinstance(pyramid_dtype, torch.dtype) or pyramid_dtype not in _PYR_FMAP_DTYPES:
        raise ValueError("pyramid_dtype must be None, torch.float32 or torch.float16; "
                         f"got {pyramid_dtype!r}")
    if fmap_dtype not in _PYR_FMAP_DTYPES:
        raise ValueError(f"pyramid_dtype={pyramid_dtype} contradicts {fmap_dtype} fmaps (it "
                         "applies to float32 and float16 fmaps; bfloat16 fmaps build a bfloat16 "
                         "pyramid)")
    return pyramid_dtype == torch.float16


_PACKED_CACHE: dict = {}


def _packed_weight(weight: torch.Tensor, device: torch.device) -> torch.Tensor:
    """A [Cout, Cin] conv weight in the fused kernel's operand layout
    (dxr_conv1x1_pack_weight), cached per (storage, version, shape) so the 12 GRU
    iterations pack it once."""
    key = (weight.data_ptr(), weight._version, tuple(weight.shape), weight.dtype, str(device))
    hit = _PACKED_CACHE.get(key)
    if hit is not None:
        return hit[1]
    cout, cin = (int(s) for s in weight.shape)
    w = weight.detach().float().contiguous()
    lib = nat.load()
    planes = torch.empty(lib.dxr_conv1x1_packed_bytes(cout, cin), dtype=torch.uint8, device=device)
    with _Launch(device):
        st = lib.dxr_conv1x1_pack_weight(w.data_ptr(), cout, cin, planes.data_ptr(),
                                          nat.stream_of(w))
    nat.check(st, "conv1x1 weight packing (dxr_conv1x1_pack_weight)")
    if len(_PACKED_CACHE) > 16:
        _PACKED_CACHE.clear()
    _PACKED_CACHE[key] = (weight, planes)   # keeps the weight alive: its pointer stays unique
    return planes


class CorrBlock:
    """All-pairs correlation pyramid + radius-r lookup (reference core/corr.py:12-60).

    ``CorrBlock(fmap1, fmap2, num_levels=4, radius=4)`` builds the pyramid of
    ``fmap1^T fmap2 / sqrt(D)`` with its avg-pool levels fused into the GEMM's
    epilogue (``dxr_corr_pyramid_build_ws``, with a workspace from torch's
    caching allocator); each ``__call__(coords)`` is one lookup launch
    (``dxr_corr_lookup``) returning a new contiguous float32
    ``[B, num_levels*(2r+1)^2, H, W]`` tensor in the reference's channel order.
    ``__call__(coords, out_dtype=torch.float16)`` (or bfloat16; also
    ``lookup_conv1x1``) stores that tensor in 16 bits from the same launch, for
    update blocks that run under autocast: the float32 result's ``.to(dtype)``
    bit for bit, with half the output traffic and no cast kernel.

    fp32 fmaps (the reference's dtype, core/raft.py:139-142) compute in f32
    class: a split pass scales every pixel's channel vector by a power of two
    and stores it as an f16 pair hi + lo, then the LDS-DMA build runs three f16
    MFMA products per f32 product (lo*hi, hi*lo, hi*hi) into one f32
    accumulator and undoes the scales exactly in the epilogue.  A workgroup
    whose sums are not finite (inf/NaN operands) recomputes its pages on the
    exact-f32 MFMA.  The pyramid is stored in f32; bf16 fmaps build a bf16
    pyramid on bf16 MFMA.  It lives in one paged buffer (``_buf``);
    ``corr_pyramid`` gives the reference-layout levels on demand.

    float16 fmaps (what the encoders emit under ``--mixed_precision``; the
    reference widens them with ``.float()``, core/raft.py:139-142) are taken as
    they are: the same LDS-DMA build on f16 records runs ONE f16 MFMA product
    per channel pair, with no split pass and no scales, into an f32 pyramid.
    Every f16 value is an f32 value and f16 x f16 products are exact in the f32
    accumulator, so this is the reference's f32 matmul on the widened fmaps to
    accumulation rounding (f32 class, unlike the bf16 mode).  Shapes that build
    does not cover (D % 32 != 0) are widened here and take the f32 path.
    Inference only: float16 fmaps that require grad raise, as bfloat16 ones do.

    ``pyramid_dtype`` (an extension: the reference constructor has no such
    argument, and ``inspect.signature`` reports the reference's four) is None by
    default, which keeps all of the above.  ``pyramid_dtype=torch.float16`` with
    float16 or float32 fmaps stores the pyramid in float16 (``DXR_PYR_F16``):
    every cell of every level is the float32 pyramid's cell for the same fmaps
    rounded once to nearest even — ``level.half()`` of the default block's
    levels, bit for bit (overflow to +-inf beyond 65504, subnormals kept) — from
    the same build kernels' own stores; lookups widen the cells on load and run
    the float32 arithmetic, so their results are the float32 lookup of the
    widened pyramid, bit for bit.  Half the pyramid memory, half the build's
    stores and half the bytes a lookup gathers, at 11 significant bits (under
    autocast the lookup tensor is rounded to float16 before ``convc1`` anyway).
    Shapes the fused build does not cover (D % 16 != 0) build the float32
    pyramid into a temporary and convert it level by level.  ``torch.float32``
    names the default of float32 / float16 fmaps; other values, or one that
    contradicts the fmap dtype (bfloat16 fmaps), raise ``ValueError``.  Inference
    only: fmaps that require grad (under grad mode) and more than 4 levels raise
    ``NotImplementedError`` before any launch.
    """

    def __init__(self, fmap1, fmap2, num_levels=4, radius=4, pyramid_dtype=None):
        self.num_levels = num_levels
        self.radius = radius
        B, D, H, W = _fmap_geometry(fmap1, fmap2)
        self._token = None
        self._gs = None
        if not isinstance(num_levels, int) or num_levels < 1:
            raise ValueError(f"num_levels must be a positive int, got {num_levels!r}")
        if not isinstance(radius, int) or radius < 0:
            raise ValueError(f"radius must be a non-negative int, got {radius!r}")
        sizes = _level_sizes(H, W, num_levels)
        if fmap1.dtype == torch.float32:
            in_dt, pyr_dt, pyr_torch = nat.DXR_F32, nat.DXR_F32, torch.float32
        elif fmap1.dtype == torch.bfloat16:
            in_dt, pyr_dt, pyr_torch = nat.DXR_BF16, nat.DXR_BF16, torch.bfloat16
        elif fmap1.dtype == torch.float16:
            in_dt, pyr_dt, pyr_torch = nat.DXR_F16, nat.DXR_F32, torch.float32
        else:
            raise RuntimeError(f"fmaps must be float32, bfloat16 or float16, got {fmap1.dtype}")
        if in_dt != nat.DXR_F32:
            _require_no_grad(fmap1, fmap2, what=f"{str(fmap1.dtype)[6:]} fmaps")
        pyr16 = _f16_pyramid(fmap1.dtype, pyramid_dtype)
        if pyr16:
            # a rounded forward with an exact backward is not offered silently
            _require_no_grad(fmap1, fmap2, what="a float16 pyramid (pyramid_dtype=torch.float16)")
            if num_levels > 4:
                raise NotImplementedError(
                    "dexiraft_amd: a float16 pyramid has at most 4 levels (levels beyond the "
                    f"fused four are pooled in float32); got num_levels={num_levels}")
            pyr_dt, pyr_torch = nat.DXR_PYR_F16, torch.float16
        self._geom = (B, D, H, W)
        self._pyr_dt = pyr_dt
        self._device = fmap1.device
        lib = nat.load()
        numel = lib.dxr_pyramid_numel(B, H, W, num_levels)
        self._buf = torch.empty(numel, dtype=pyr_torch, device=fmap1.device)
        grad = _wants_grad(fmap1, fmap2)
        self._in_dt = in_dt
        f1, f2, st = self._launch_build(fmap1, fmap2, grad)
        if st == nat.DXR_EUNSUPPORTED and in_dt == nat.DXR_F16:
            # a shape the f16 record build does not cover (D % 32 != 0): widen
            # exactly, as the reference does (core/raft.py:139-142), and take the
            # f32 path; the memory format is kept
            self._in_dt = nat.DXR_F32
            f1, f2, st = self._launch_build(fmap1.float(), fmap2.float(), grad)
        if st == nat.DXR_EUNSUPPORTED and pyr16:
            st = self._build_f16_pyramid_from_f32(fmap1, fmap2)
        nat.check(st, "CorrBlock build (dxr_corr_pyramid_build_ws)")
        self._level_sizes = sizes
        self._ref_pyramid = None
        if grad:
            self._gs = _GradState(self._geom, num_levels, radius, self._device, numel)
            self._token = _BuildGrad.apply(f1, f2, self._gs)

    def _build_f16_pyramid_from_f32(self, fmap1, fmap2):
        """The float16 pyramid of a shape the fused float16-store builds do not
        cover (D % 16 != 0): the float32 pyramid of the widened fmaps, built into
        a temporary by the default path, then rounded level by level
        (``dxr_pyramid_unpack`` + ``dxr_pyramid_pack(..., DXR_PYR_F16)``) — by
        definition the same pyramid.  Pack writes no padding cell, so the buffer
        is zero-filled first.  Returns the status."""
        B, D, H, W = self._geom
        lib = nat.load()
        self._in_dt = nat.DXR_F32
        tmp = torch.empty(self._buf.numel(), dtype=torch.float32, device=self._device)
        _, _, st = self._launch_build(fmap1.float(), fmap2.float(), False, buf=tmp,
                                      pyr_dt=nat.DXR_F32)
        if st != nat.DXR_OK:
            return st
        self._buf.zero_()
        with _Launch(self._device):
            for lvl, (h, w) in enumerate(_level_sizes(H, W, self.num_levels)):
                t = torch.empty((B * H * W, h, w), dtype=torch.float32, device=self._device)
                st = lib.dxr_pyramid_unpack(tmp.data_ptr(), nat.DXR_F32, B, H, W, self.num_levels,
                                            lvl, t.data_ptr(), nat.stream_of(t))
                if st != nat.DXR_OK:
                    return st
                st = lib.dxr_pyramid_pack(t.data_ptr(), B, H, W, self.num_levels, lvl,
                                          self._buf.data_ptr(), nat.DXR_PYR_F16, nat.stream_of(t))
                if st != nat.DXR_OK:
                    return st
        return nat.DXR_OK

    def _launch_build(self, fmap1, fmap2, grad=False, buf=None, pyr_dt=None):
        """One build launch into this block's pyramid buffer (or ``buf``, a
        pyramid of ``pyr_dt``).  Returns the operand tensors the kernel read and
        the status.

        f32 fmaps get a workspace from torch's caching allocator (freed when the
        build's stream work is done) for the pre-split build
        (``dxr_corr_pyramid_build_ws``: operands scaled and split into f16 pairs
        once, then moved by LDS-DMA)."""
        B, D, H, W = self._geom
        lib = nat.load()
        nbytes = max(lib.dxr_build_workspace_bytes(self._in_dt, B, D, H, W), 0)
        buf = self._buf if buf is None else buf
        pyr_dt = self._pyr_dt if pyr_dt is None else pyr_dt

        def launch(f1, f2, layout, with_ws=True):
            ws = torch.empty(nbytes, dtype=torch.uint8, device=self._device) \
                if with_ws and nbytes > 0 else None
            with _Launch(self._device):
                return lib.dxr_corr_pyramid_build_ws(
                    f1.data_ptr(), f2.data_ptr(), self._in_dt, layout, B, D, H, W,
                    self.num_levels, _sqrt_dim(D), buf.data_ptr(), pyr_dt,
                    nat.DXR_BUILD_AUTO, nat.ptr(ws), nbytes if ws is not None else 0,
                    nat.stream_of(f1))

        st = nat.DXR_EUNSUPPORTED
        if not grad and _channels_last(fmap1) and _channels_last(fmap2):
            # channels-last fmaps: read in place by the
            # build's NHWC operand loads (f32: the pre-split pass, into the
            # workspace; bf16 / f16: the DMA build reads the rows directly and
            # needs no workspace), no layout pass
            f1, f2 = fmap1, fmap2
            st = launch(f1, f2, nat.DXR_NHWC, with_ws=self._in_dt == nat.DXR_F32)
        if st == nat.DXR_EUNSUPPORTED:
            if grad:
                f1, f2 = fmap1.contiguous(), fmap2.contiguous()   # tracked by autograd
            else:
                f1, f2 = _nchw(fmap1), _nchw(fmap2)
            st = launch(f1, f2, nat.DXR_NCHW)
        return f1, f2, st

    @property
    def corr_pyramid(self):
        """Reference-layout levels ``[B*H*W, 1, H_l, W_l]`` (core/corr.py:16-27).

        The native pyramid is stored paged (one contiguous page per build
        workgroup, include/dexiraft_corr.h); this list is materialised on first
        access by ``dxr_pyramid_unpack`` and cached.  Values are float32 (bf16
        and float16 pyramids are widened).  The lookup never needs it.
        """
        if self._ref_pyramid is None:
            B, D, H, W = self._geom
            lib = nat.load()
            levels = []
            with _Launch(self._device):
                for lvl, (h, w) in enumerate(self._level_sizes):
                    t = torch.empty((B * H * W, 1, h, w), dtype=torch.float32, device=self._device)
                    st = lib.dxr_pyramid_unpack(self._buf.data_ptr(), self._pyr_dt, B, H, W,
                                                self.num_levels, lvl, t.data_ptr(),
                                                nat.stream_of(t))
                    nat.check(st, "CorrBlock.corr_pyramid (dxr_pyramid_unpack)")
                    levels.append(t)
            self._ref_pyramid = levels
        return self._ref_pyramid

    def __call__(self, coords, out_dtype=None, *, memory_format=None):
        """The radius-r lookup around ``coords``: ``[B, num_levels*(2r+1)^2, H, W]``.

        ``memory_format``: None or ``torch.contiguous_format`` (the default: a
        contiguous NCHW tensor, as the reference) or ``torch.channels_last``: the
        same shape and the same elements bit for bit, in a tensor allocated
        channels-last that the kernel fills in place (``DXR_OUT_NHWC``) — what a
        channels-last update block would otherwise produce with a layout copy
        before ``convc1``.  Anything else raises ``ValueError``.  The backward
        is unchanged (it reads ``grad_out.contiguous()``).

        ``out_dtype``: None or torch.float32 (the default: float32, as the
        reference), torch.float16 or torch.bfloat16 (anything else raises
        ``ValueError``).  A 16-bit result is ``self(coords).to(out_dtype)`` bit
        for bit — the float32 sums, rounded to nearest even in the kernel's own
        stores (float16: overflow to +-inf, subnormals kept; NaNs stay NaNs) —
        i.e. the cast autocast applies before ``convc1`` (core/update.py:90),
        without the float32 tensor and the cast kernel.  Under grad the
        backward is the float32 lookup's, fed ``grad_out.float()``.
        """
        B, D, H, W = self._geom
        _out_flag(out_dtype)
        _layout_flag(memory_format)
        _require_no_grad(coords, what="coords (the reference detaches them, core/raft.py:170)")
        c = _check_coords(coords, B, H, W, self._device)
        if self._token is not None and torch.is_grad_enabled():
            return _LookupGrad.apply(self._token, c, self, out_dtype, memory_format)
        return self._lookup(c, out_dtype, memory_format)

    # Introspection (inspect.signature, help()) reports the reference's own
    # ``__call__(self, coords)`` (core/corr.py:29): the class is a drop-in and its
    # declared surface is pinned to the reference's (tests/test_api_cpu.py).
    # ``out_dtype`` and ``memory_format`` are extensions on top of it, optional and documented above;
    # callers that never pass it get the reference's behaviour.
    __call__.__signature__ = inspect.Signature([
        inspect.Parameter("self", inspect.Parameter.POSITIONAL_OR_KEYWORD),
        inspect.Parameter("coords", inspect.Parameter.POSITIONAL_OR_KEYWORD)])
    # The same for the constructor (core/corr.py:13): ``pyramid_dtype`` is an
    # extension on top of the reference's four arguments (class docstring).
    __init__.__signature__ = inspect.Signature([
        inspect.Parameter("self", inspect.Parameter.POSITIONAL_OR_KEYWORD),
        inspect.Parameter("fmap1", inspect.Parameter.POSITIONAL_OR_KEYWORD),
        inspect.Parameter("fmap2", inspect.Parameter.POSITIONAL_OR_KEYWORD),
        inspect.Parameter("num_levels", inspect.Parameter.POSITIONAL_OR_KEYWORD, default=4),
        inspect.Parameter("radius", inspect.Parameter.POSITIONAL_OR_KEYWORD, default=4)])

    def _lookup(self, c, out_dtype=None, memory_format=None):
        B, D, H, W = self._geom
        rd = 2 * self.radius + 1
        out_torch, flag = _out_flag(out_dtype)
        layout = _layout_flag(memory_format)
        flag |= layout
        out = _empty_out((B, self.num_levels * rd * rd, H, W), out_torch, self._device, layout)
        lib = nat.load()
        with _Launch(self._device):
            st = lib.dxr_corr_lookup(self._buf.data_ptr(), self._pyr_dt | flag, B, H, W,
                                     self.num_levels, self.radius, c.data_ptr(),
                                     out.data_ptr(), nat.stream_of(c))
        nat.check(st, "CorrBlock lookup (dxr_corr_lookup)")
        return out

    def lookup_conv1x1(self, coords, weight, bias=None, relu=True, out_dtype=None, *,
                       memory_format=None):
        """Lookup fused with the motion encoder's first 1x1 convolution:
        ``F.relu(F.conv2d(self(coords), weight, bias))`` in one launch
        (``dxr_corr_lookup_conv1x1``).

        Replaces ``corr = corr_fn(coords1)`` (core/raft.py:172) followed by
        ``cor = F.relu(self.convc1(corr))`` in BasicMotionEncoder.forward
        (core/update.py:90; SmallMotionEncoder :71): pass ``convc1.weight`` and
        ``convc1.bias``.  Returns a new contiguous float32 ``[B, Cout, H, W]``
        (``out_dtype`` torch.float16 / torch.bfloat16: that dtype, equal to the
        float32 result's ``.to(out_dtype)`` bit for bit — same accumulation, bias
        and ReLU in float32, only the store converts; other values as in
        ``__call__``).  ``memory_format=torch.channels_last``: the same shape and
        elements in a channels-last tensor, stored so by the kernel (as
        ``__call__``).
        The samples are bit-identical to ``__call__``'s; the contraction runs in
        f32 class on the matrix cores while operand magnitudes (weights and
        samples) are at least 2^-13: both are split into float16 pairs without a
        prescale, so a smaller operand is carried with an absolute resolution of
        2^-36 instead of a relative 2^-22.  A workgroup (32 consecutive pixels of
        one batch item) whose sums are not finite, e.g. because an operand of
        65520 or more is inf in float16, repeats its contraction on a three-way
        bfloat16 split with float32's range.  The per-element bound is derived in
        tests/motion_oracle.py.  Inference only (raises under grad for
        inputs that require grad).  Supported: radius 3/4, num_levels <= 4,
        Cout a multiple of 32 (the reference's 256 and 96).
        """
        B, D, H, W = self._geom
        out_torch, flag = _out_flag(out_dtype)
        layout = _layout_flag(memory_format)
        flag |= layout
        _require_no_grad(coords, weight, *(() if bias is None else (bias,)),
                         what="CorrBlock.lookup_conv1x1 (inference fusion)")
        if self._token is not None and torch.is_grad_enabled():
            raise NotImplementedError("CorrBlock.lookup_conv1x1 is inference-only; call the "
                                      "block and convc1 separately to train through them")
        c = _check_coords(coords, B, H, W, self._device)
        rd = 2 * self.radius + 1
        cin = self.num_levels * rd * rd
        _require_device(weight, "weight")
        if weight.dim() == 4 and tuple(weight.shape[2:]) == (1, 1):
            weight = weight.reshape(weight.shape[0], weight.shape[1])
        if weight.dim() != 2 or int(weight.shape[1]) != cin:
            raise RuntimeError(f"weight must be [Cout, {cin}, 1, 1] (or [Cout, {cin}]), "
                               f"got {tuple(weight.shape)}")
        cout = int(weight.shape[0])
        if bias is not None:
            _require_device(bias, "bias")
            if tuple(bias.shape) != (cout,):
                raise RuntimeError(f"bias must be [{cout}], got {tuple(bias.shape)}")
            bias = bias.detach().float().contiguous()
        planes = _packed_weight(weight, self._device)
        out = _empty_out((B, cout, H, W), out_torch, self._device, layout)
        lib = nat.load()
        with _Launch(self._device):
            st = lib.dxr_corr_lookup_conv1x1(self._buf.data_ptr(), self._pyr_dt | flag, B, H, W,
                                             self.num_levels, self.radius, c.data_ptr(),
                                             planes.data_ptr(), nat.ptr(bias), cout, int(bool(relu)),
                                             out.data_ptr(), nat.stream_of(c))
        nat.check(st, "CorrBlock.lookup_conv1x1 (dxr_corr_lookup_conv1x1)")
        return out

    # ``memory_format`` (keyword-only) is an extension in the same way: the
    # declared surface stays the one ``out_dtype`` introduced.
    lookup_conv1x1.__signature__ = inspect.Signature(
        [inspect.Parameter(n, inspect.Parameter.POSITIONAL_OR_KEYWORD, default=d)
         for n, d in (("self", inspect.Parameter.empty), ("coords", inspect.Parameter.empty),
                      ("weight", inspect.Parameter.empty), ("bias", None), ("relu", True),
                      ("out_dtype", None))])

    @staticmethod
    def corr(fmap1, fmap2):
        """``[B, H, W, 1, H, W]`` volume ``fmap1^T fmap2 / sqrt(D)`` (core/corr.py:52-60);
        differentiable in the fmaps under grad mode."""
        _fmap_geometry(fmap1, fmap2)
        if _wants_grad(fmap1, fmap2) and fmap1.dtype == torch.float32:
            return _VolumeGrad.apply(fmap1.contiguous(), fmap2.contiguous())
        return CorrBlock._volume(fmap1, fmap2)

    @staticmethod
    def _volume(fmap1, fmap2):
        B, D, H, W = _fmap_geometry(fmap1, fmap2)
        if fmap1.dtype != torch.float32:
            raise RuntimeError(f"CorrBlock.corr expects float32 fmaps, got {fmap1.dtype}")
        out = torch.empty((B, H, W, 1, H, W), dtype=torch.float32, device=fmap1.device)
        f1, f2 = _nchw(fmap1), _nchw(fmap2)
        lib = nat.load()
        with _Launch(fmap1.device):
            st = lib.dxr_corr_volume(f1.data_ptr(), f2.data_ptr(), nat.DXR_F32, B, D, H, W,
                                     _sqrt_dim(D), out.data_ptr(), nat.stream_of(f1))
        nat.check(st, "CorrBlock.corr (dxr_corr_volume)")
        return out


class AlternateCorrBlock:
    """On-the-fly correlation lookup (reference core/corr.py:63-91 + alt_cuda_corr).

    Memory is O(H*W*D) at the fine levels instead of O((H*W)^2): only pooled fmaps
    are kept and each ``__call__`` computes the (2r+2)^2 window dot products of
    those levels in one launch (``dxr_alt_corr_lookup_levels_ws``), divided by
    sqrt(D).  Round 6: on large maps (``COARSE_MIN_QUERIES``) the coarse levels —
    from the first level of at most ``COARSE_LEVEL_MAX_CELLS`` cells on, within
    ``COARSE_VOLUME_MAX_BYTES`` — are computed once per block as whole volumes of the
    same dot products (``dxr_alt_coarse_volumes``, one tiled GEMM per level) and read
    by ``dxr_alt_volume_lookup``: an on-the-fly lookup pays each level's box GEMMs
    again on every call (~15-26 us per coarse level at 1080p), while a coarse
    level's whole volume costs about one or two calls (1080p: levels 2-3).
    With finite operands in the f16 pair's range the outputs are the all-on-the-
    fly form's bit for bit (``coarse_first_level`` None: no volumes).  As in the
    reference, the constructor pools ``num_levels`` times, so fmaps smaller than
    2^num_levels in either dimension raise (core/corr.py:69-71).
    16-bit fmaps are read in place, where the reference widens them to float32
    first (its own cast, core/raft.py:139-142).  float16 fmaps — what the encoders emit under
    ``--mixed_precision`` — are read in place (``NATIVE_F16``; D % 16 == 0,
    D <= 256, radius <= 6): the block keeps fmap1 and fmap2 level 0 as float16
    NHWC (a free view of channels-last fmaps), pools level 1 from a transient
    float32 copy of level 0 and the further levels from float32 as ever, and its
    lookups pass ``DXR_ALT_IN_F16``: level 0 is one f16 matrix-core product per k
    step on the raw values, the pooled levels two instead of three.  With finite
    fmaps every output equals (``torch.equal``) that of the block built on
    ``fmap1.float(), fmap2.float()``, under every ``out_dtype`` /
    ``memory_format`` and with or without coarse volumes (those are computed once
    from a transient float32 fmap1, unchanged); the block then holds no float32
    copy of the fmaps.  With ``NATIVE_F16 = False``, for other D or radius, or if
    the library declines the flag (``DXR_EUNSUPPORTED``: the operands are widened
    once and the block goes on as before), float16 fmaps are widened exactly to
    float32 in the constructor.
    bfloat16 fmaps — the usual autocast dtype — are read in place in the same way
    (``NATIVE_BF16``, the same D and radius; ``DXR_ALT_IN_BF16``): the same
    bfloat16 NHWC operands, float32 pooled levels (bit for bit the widened
    block's), transient float32 copies for level 1 and the coarse volumes (those
    are the widened block's bit for bit), and the same fallbacks.  Level 0 is one
    bf16 matrix-core product per k step on the raw values — exact products,
    float32's exponent range: no split, no scaling, no overflow fallback — and a
    pooled level three exact products (its float32 cells split three ways, times
    the raw query).  Unlike the float16 form this one is not bit-equal to the
    widened block: the same exact products are summed by another instruction (and
    the widened block recomputes values outside float16's range on its fallback).
    Every output is within 1e-5 of sum |fmap1| |fmap2| of the exact result (the
    criterion of tests/test_gpu_alt_oracle.py), the ordered and tile-order forms
    agree bit for bit, and every ``out_dtype`` / ``memory_format`` output is the
    block's own float32 NCHW output converted.

    ``out_dtype`` (None / torch.float32, torch.float16, torch.bfloat16) and
    ``memory_format`` (None / torch.contiguous_format, torch.channels_last) are
    keyword-only constructor arguments — the consumer is the same for all of a block's
    lookups — and anything else raises ``ValueError`` before the native library
    is reached; ``__call__(coords)`` keeps the reference's signature.  Every
    lookup then returns ``[B, num_levels*(2r+1)^2, H, W]`` of that dtype with
    those strides, equal bit for bit to the default block's float32 contiguous
    result converted with ``.to(out_dtype)`` /
    ``.contiguous(memory_format=torch.channels_last)``: the kernels store it so
    themselves (``DXR_OUT_F16`` / ``DXR_OUT_BF16`` / ``DXR_OUT_NHWC`` on the
    ``radius`` argument of the native calls; the float32 sums rounded to nearest
    even in the store, float16 overflow to +-inf, NaN bits as torch's conversion
    gives them), without the float32 tensor,
    the cast kernel or the layout copy.  The MFMA forms (D % 16 == 0, D <= 256:
    every RAFT model) and the volume lookup do this natively; for other D the
    library declines the flags (``DXR_EUNSUPPORTED``) and ``_lookup`` runs the
    float32 NCHW call and converts with torch — the same tensor by definition.

    Memory of the coarse volumes.  A block with volumes holds, beside its
    O(H*W*D) operands, ``dxr_alt_volume_numel`` cells: about 333 MB of float32 per
    1080p pair (levels 2-3, B = 1; about 1 GB at B = 3), up to the 1 GiB cap
    ``COARSE_VOLUME_MAX_BYTES``, beyond which a level or all volumes are dropped
    and those levels run on the fly.  ``volume_dtype`` (keyword-only; None /
    torch.float32: as described so far, torch.float16; anything else raises
    ``ValueError`` before the fmaps are looked at) selects float16 volumes, half
    that memory.  No new tolerance: every cell is the float32 volume's cell
    rounded once to float16 (to nearest even, beyond 65504 to +-inf, subnormals
    kept; the volume GEMM stores them so itself, ``DXR_ALT_VOL_F16``), a lookup
    widens cells on load (exact) and runs the float32 arithmetic, so every
    output is that of a float32-volume block whose volumes are
    ``.half().float()`` of themselves, bit for bit, under every ``out_dtype`` /
    ``memory_format``; the on-the-fly levels ``[0, coarse_first_level)`` are
    untouched.  Against the float32-volume block a coarse level's outputs differ
    by at most ((2^-11 + 2^-21) Vmax + 2^-25) / sqrt(D), Vmax the level's largest
    |cell|.  The cap counts the volumes' real bytes, so a float16 block may keep a
    level or a batch the float32 block drops.  The GEMM serves D % 32 == 0 and at
    most 4 levels; otherwise (``DXR_EUNSUPPORTED``) the block builds the float32
    volumes and keeps their ``.half()`` — the same buffer by definition, with a
    transient peak of 1.5 times the float32 volumes during construction.  It works
    with float32, float16 and bfloat16 fmaps (the volumes come from the transient
    float32 fmap1 as before).  A block without volumes (small maps) accepts and
    ignores the argument; the read-only ``volume_dtype`` reports what the block
    holds (None without volumes).
    The volumes are computed in the constructor: the fmaps must not be modified
    after construction (the volumes would go stale, and channels-last fmaps are
    read in place by every lookup).
    """

    # Which levels are precomputed (round 6, bench.py --block alt, profiles/r06/experiments/
    # r6n_*): at 1080p (32,640 queries) levels 2-3 (2,040 + 510 cells) as volumes take the
    # lookup from 164.1 to 127.2 us for ~200 us per block (tiled GEMM: level 2 149 us, level 3
    # 42 us): 498.9 -> 568.0 pairs/s (+13.9 %; level 3 alone 536.8); at Sintel (7,040
    # queries) the on-the-fly coarse levels cost ~2-4 us per lookup and volumes lose 3-4 %.
    COARSE_LEVEL_MAX_CELLS = 2048          # a level of at most this many cells is precomputed
    COARSE_MIN_QUERIES = 16384             # on maps of at least this many query pixels
    COARSE_VOLUME_MAX_BYTES = 1 << 30      # and all precomputed volumes fit in this
    # The volume GEMM's LDS-DMA form on pre-split f16 pair planes (dxr_alt_coarse_volumes_ws):
    # bit-identical, 6 % faster isolated, but 1.2 % slower in the 1080p step (r6u: 563 vs 570
    # pairs/s, two rounds each on one box), so off.
    COARSE_VOLUME_PLANES = False
    # float16 fmaps are read in place (DXR_ALT_IN_F16; class docstring).  False: they are
    # widened in the constructor like bfloat16 ones — the same outputs from float32 copies
    # (scripts/ab_alt_f16.py compares the two; profiles/r14/alt_f16).
    NATIVE_F16 = True
    # bfloat16 fmaps are read in place (DXR_ALT_IN_BF16; class docstring).  False: they are
    # widened in the constructor, call for call as before the flag existed
    # (scripts/ab_alt_bf16.py compares the two; profiles/r15/alt_bf16).
    NATIVE_BF16 = True

    def __init__(self, fmap1, fmap2, num_levels=4, radius=4, *, out_dtype=None,
                 memory_format=None, **extensions):
        volume_dtype = _pop_volume_dtype(extensions)
        self.num_levels = num_levels
        self.radius = radius
        self._out_torch, self._out_flags = _out_flag(out_dtype)
        self._vol16 = _f16_volumes(volume_dtype)
        self._out_layout = _layout_flag(memory_format)
        self._out_flags |= self._out_layout
        self._out_native = True   # until the library declines the flags (a VALU form)
        B, D, H, W = _fmap_geometry(fmap1, fmap2)
        _require_no_grad(fmap1, fmap2, what="AlternateCorrBlock (the reference's alt_cuda_corr "
                                            "output carries no autograd graph, core/corr.py:85-88)")
        # 16-bit fmaps in place: until the library declines DXR_ALT_IN_F16 / DXR_ALT_IN_BF16
        # (_in16: float16 operands; _inbf16: bfloat16 operands)
        served = isinstance(radius, int) and 0 <= radius <= 6 and D % 16 == 0 and D <= 256
        self._in16 = bool(self.NATIVE_F16 and fmap1.dtype == torch.float16 and served)
        self._inbf16 = bool(self.NATIVE_BF16 and fmap1.dtype == torch.bfloat16 and served)
        if self._in16 or self._inbf16:
            pass   # kept as they are
        elif fmap1.dtype in (torch.bfloat16, torch.float16):
            # The reference computes in float32 (core/raft.py:139-142 casts the
            # fmaps; alt_cuda_corr is float-only): bf16 / f16 encoder outputs are
            # widened exactly, keeping their memory format (channels-last stays a
            # free view).
            fmap1, fmap2 = fmap1.float(), fmap2.float()
        elif fmap1.dtype != torch.float32:
            raise RuntimeError(f"AlternateCorrBlock expects float32, bfloat16 or float16 fmaps, "
                               f"got {fmap1.dtype}")
        if not isinstance(num_levels, int) or num_levels < 1:
            raise ValueError(f"num_levels must be a positive int, got {num_levels!r}")
        if not isinstance(radius, int) or radius < 0:
            raise ValueError(f"radius must be a non-negative int, got {radius!r}")
        _level_sizes(H, W, num_levels + 1)  # the reference pools num_levels times
        self._geom = (B, D, H, W)
        self._device = fmap1.device
        # NHWC operands (core/corr.py:82-83 permutes on every call; here once per
        # block): a free view of channels-last fmaps, one tiled transpose otherwise.
        # Only full-res fmap1 and the pooled fmap2 levels are used (core/corr.py:82-83),
        # so only those are pooled; ``pyramid`` materialises the rest on demand.
        # (16-bit in place: no reference to the caller's fmaps; ``pyramid`` widens the
        # NHWC operands into tensors of the caller's memory formats)
        self._fmaps = None if self._in16 or self._inbf16 else (fmap1, fmap2)
        self._fmaps_cl = (_channels_last(fmap1), _channels_last(fmap2))
        self._pyramid = None
        self._f1_nhwc = _nhwc(fmap1)
        self._f2_nhwc = [_nhwc(fmap2)]
        for l in range(1, num_levels):
            # (16-bit level 0: level 1 is pooled from a transient float32 copy, bit for bit
            # the widened block's; the means are not 16-bit numbers and stay float32)
            above = self._f2_nhwc[-1]
            self._f2_nhwc.append(_pool_nhwc(above.float() if l == 1 else above))
        self._f2_ptrs = (ctypes.c_void_p * num_levels)(*[t.data_ptr() for t in self._f2_nhwc])
        self.coarse_first_level = None
        self._volumes = None
        if D % 16 == 0 and D <= 256 and radius <= 6 and B > 0 and H * W >= self.COARSE_MIN_QUERIES:
            self._make_volumes(B, D, H, W)

    # Introspection reports the reference's constructor (core/corr.py:64), as
    # CorrBlock's does: ``out_dtype``, ``memory_format`` and ``volume_dtype`` are extensions
    # on top of its four arguments (class docstring; tests/test_api_cpu.py).
    __init__.__signature__ = inspect.Signature([
        inspect.Parameter("self", inspect.Parameter.POSITIONAL_OR_KEYWORD),
        inspect.Parameter("fmap1", inspect.Parameter.POSITIONAL_OR_KEYWORD),
        inspect.Parameter("fmap2", inspect.Parameter.POSITIONAL_OR_KEYWORD),
        inspect.Parameter("num_levels", inspect.Parameter.POSITIONAL_OR_KEYWORD, default=4),
        inspect.Parameter("radius", inspect.Parameter.POSITIONAL_OR_KEYWORD, default=4)])

    def _make_volumes(self, B, D, H, W):
        lib = nat.load()
        sizes = _level_sizes(H, W, self.num_levels)
        first = next((lvl for lvl in range(1, self.num_levels)
                      if sizes[lvl][0] * sizes[lvl][1] <= self.COARSE_LEVEL_MAX_CELLS), None)
        while first is not None and first < self.num_levels:
            n = lib.dxr_alt_volume_numel(B, H, W, self.num_levels, first)
            if 0 < n * (2 if self._vol16 else 4) <= self.COARSE_VOLUME_MAX_BYTES:   # real bytes
                break
            first += 1
        if first is None or first >= self.num_levels:
            return
        vol = torch.empty((n,), dtype=torch.float16 if self._vol16 else torch.float32,
                          device=self._device)
        vflag = nat.DXR_ALT_VOL_F16 if self._vol16 else 0
        # with COARSE_VOLUME_PLANES, the f16 pair planes of the operands (the volume GEMM's
        # LDS-DMA form), from torch's caching allocator: freed once the launches that read
        # them have run; 0 bytes: the register form
        nbytes = (lib.dxr_alt_coarse_volumes_ws_bytes(B, H, W, D, self.num_levels, first)
                  if self.COARSE_VOLUME_PLANES else 0)
        ws = torch.empty(max(nbytes, 0), dtype=torch.uint8, device=self._device)
        # (16-bit in place: the volume GEMM reads a transient float32 fmap1 and the float32
        # pooled levels >= first >= 1 — the widened block's call, bit for bit)
        f1 = self._f1_nhwc.float()   # (a no-op on float32 operands)
        with _Launch(self._device):
            st = lib.dxr_alt_coarse_volumes_ws(f1.data_ptr(), self._f2_ptrs, B, H, W, D,
                                               self.num_levels, first | vflag, vol.data_ptr(),
                                               nat.ptr(ws), max(nbytes, 0), nat.stream_of(vol))
            if vflag and st == nat.DXR_EUNSUPPORTED:
                # D % 32 != 0 or more than 4 levels (the FULL form and row-major levels store
                # float32): the float32 volumes, rounded once — the same buffer by definition.
                # Transient peak: the float32 volumes beside their float16 copy, 1.5 times the
                # float32 block's volume memory, until the float32 buffer is freed below.
                vol32 = torch.empty((n,), dtype=torch.float32, device=self._device)
                st = lib.dxr_alt_coarse_volumes_ws(f1.data_ptr(), self._f2_ptrs, B, H, W, D,
                                                   self.num_levels, first, vol32.data_ptr(),
                                                   nat.ptr(ws), max(nbytes, 0),
                                                   nat.stream_of(vol))
                if st == nat.DXR_OK:
                    vol.copy_(vol32)
                del vol32
        nat.check(st, "AlternateCorrBlock coarse volumes (dxr_alt_coarse_volumes_ws)")
        self.coarse_first_level = first
        self._volumes = vol

    @property
    def volume_dtype(self):
        """dtype of the coarse volumes the block holds (None: no volumes)."""
        return None if self._volumes is None else self._volumes.dtype

    @property
    def pyramid(self):
        """The reference's ``pyramid`` (core/corr.py:66-72): ``num_levels + 1`` pairs
        ``(fmap1_i, fmap2_i)`` of 2x2-pooled fmaps, ``[B, D, H_i, W_i]`` float32.

        Entry 0 is the caller's fmaps; the pooled entries are channels-last
        tensors (values bit-identical to F.avg_pool2d), materialised on first access
        — the lookup needs only full-res fmap1 and fmap2's first num_levels levels.
        """
        if self._pyramid is None:
            p1 = [self._f1_nhwc.float()]   # (a no-op on float32 operands)
            p2 = list(self._f2_nhwc)
            p2[0] = p2[0].float()
            while len(p1) < self.num_levels + 1:
                p1.append(_pool_nhwc(p1[-1]))
            while len(p2) < self.num_levels + 1:
                p2.append(_pool_nhwc(p2[-1]))
            fmaps = self._fmaps
            if fmaps is None:   # 16-bit fmaps read in place: widened here, on first access
                fmaps = tuple(t.permute(0, 3, 1, 2) if cl else t.permute(0, 3, 1, 2).contiguous()
                              for t, cl in zip((p1[0], p2[0]), self._fmaps_cl))
            pyr = [fmaps]
            pyr += [(a.permute(0, 3, 1, 2), b.permute(0, 3, 1, 2)) for a, b in zip(p1[1:], p2[1:])]
            self._pyramid = pyr
        return self._pyramid

    def __call__(self, coords):
        B, D, H, W = self._geom
        _require_no_grad(coords, what="coords (the reference detaches them, core/raft.py:170)")
        c = _check_coords(coords, B, H, W, self._device)
        return self._lookup(c)

    def _lookup(self, c):
        # (a declined request is remembered: later lookups go straight to the fallback)
        out = self._launch_lookup(c, self._out_flags) if self._out_native else None
        if out is None:
            self._out_native = False
            # a VALU form (D % 16 != 0 or D > 256) declined the flags: the float32
            # NCHW lookup, converted — the same tensor by definition
            out = self._launch_lookup(c, 0).to(self._out_torch)
            if self._out_layout:
                out = out.contiguous(memory_format=torch.channels_last)
        return out

    def _widen_operands(self):
        """The library declined ``DXR_ALT_IN_F16`` / ``DXR_ALT_IN_BF16``: float32
        operands from here on, as the constructor makes them with ``NATIVE_F16`` /
        ``NATIVE_BF16 = False``."""
        self._in16 = self._inbf16 = False
        self._f1_nhwc = self._f1_nhwc.float()
        self._f2_nhwc[0] = self._f2_nhwc[0].float()
        self._f2_ptrs = (ctypes.c_void_p * self.num_levels)(*[t.data_ptr() for t in self._f2_nhwc])

    def _launch_lookup(self, c, flags):
        """One lookup with output ``flags`` or-ed onto the radius; None when the
        library declines a flagged request (``DXR_EUNSUPPORTED``)."""
        B, D, H, W = self._geom
        rd = 2 * self.radius + 1
        if flags:
            out = _empty_out((B, self.num_levels * rd * rd, H, W), self._out_torch, self._device,
                             self._out_layout)
        else:
            out = torch.empty((B, self.num_levels * rd * rd, H, W), dtype=torch.float32,
                              device=self._device)
        in_flag = (nat.DXR_ALT_IN_F16 if self._in16 else
                   nat.DXR_ALT_IN_BF16 if self._inbf16 else 0)
        radius = self.radius | flags | in_flag
        lib = nat.load()
        first = self.coarse_first_level
        if first is None:
            # query-order workspace (dxr_alt_corr_lookup_ws), from torch's caching
            # allocator: freed once the launches that use it have run
            nbytes = lib.dxr_alt_workspace_bytes(B, H, W, self.num_levels)
            ws = torch.empty(max(nbytes, 0), dtype=torch.uint8, device=self._device)
            with _Launch(self._device):
                st = lib.dxr_alt_corr_lookup_ws(self._f1_nhwc.data_ptr(), self._f2_ptrs,
                                                c.data_ptr(), out.data_ptr(), B, H, W, D,
                                                self.num_levels, radius, _sqrt_dim(D),
                                                nat.ptr(ws), max(nbytes, 0), nat.stream_of(c))
            if in_flag and st == nat.DXR_EUNSUPPORTED and self.radius <= 6:
                self._widen_operands()   # once: remembered, as a declined output flag is
                return self._launch_lookup(c, flags)
            if flags and st == nat.DXR_EUNSUPPORTED and self.radius <= 6:
                return None
            nat.check(st, "AlternateCorrBlock lookup (dxr_alt_corr_lookup_ws)")
            return out
        with _Launch(self._device):
            if first > 0:   # the fine levels on the fly
                nbytes = lib.dxr_alt_workspace_bytes(B, H, W, first)
                ws = torch.empty(max(nbytes, 0), dtype=torch.uint8, device=self._device)
                st = lib.dxr_alt_corr_lookup_levels_ws(self._f1_nhwc.data_ptr(), self._f2_ptrs,
                                                       c.data_ptr(), out.data_ptr(), B, H, W, D,
                                                       self.num_levels, first, radius,
                                                       _sqrt_dim(D), nat.ptr(ws), max(nbytes, 0),
                                                       nat.stream_of(c))
                if in_flag and st == nat.DXR_EUNSUPPORTED and self.radius <= 6:
                    self._widen_operands()
                    return self._launch_lookup(c, flags)
                if flags and st == nat.DXR_EUNSUPPORTED and self.radius <= 6:
                    return None
                nat.check(st, "AlternateCorrBlock lookup (dxr_alt_corr_lookup_levels_ws)")
            # (the volumes are float32 or float16 whatever the fmaps: no input flag there)
            vflag = nat.DXR_ALT_VOL_F16 if self._volumes.dtype == torch.float16 else 0
            st = lib.dxr_alt_volume_lookup(self._volumes.data_ptr(), c.data_ptr(), out.data_ptr(),
                                           B, H, W, self.num_levels, first,
                                           self.radius | flags | vflag, _sqrt_dim(D),
                                           nat.stream_of(c))
        nat.check(st, "AlternateCorrBlock lookup (dxr_alt_volume_lookup)")
        return out


class _AltLookupGrad(torch.autograd.Function):
    """Graph node of one TrainableAlternateCorrBlock lookup: differentiable in the
    fmaps only.  Saves ``coords``; everything else the backward reads is the
    block's own O(B*H*W*D) state (NHWC fmap1, the pooled fmap2 levels)."""

    @staticmethod
    def forward(ctx, fmap1, fmap2, coords, block):
        ctx.block = block
        ctx.save_for_backward(coords)
        return block._lookup(coords)

    @staticmethod
    def backward(ctx, gout):
        (coords,) = ctx.saved_tensors
        df1, df2 = ctx.block._lookup_backward(coords, gout, ctx.needs_input_grad[:2])
        return df1, df2, None, None


class TrainableAlternateCorrBlock(AlternateCorrBlock):
    """``AlternateCorrBlock`` that can be trained through: O(H*W*D) memory in the
    forward *and* in the backward (``CorrBlock``, the other trainable block, keeps
    an O((H*W)^2) pyramid and a gradient pyramid of the same size).

    Without a fmap that requires grad, or with grad mode off, every output is
    ``AlternateCorrBlock``'s bit for bit and carries no graph.  With float32 fmaps
    that require grad the forward is still the parent's (coarse volumes,
    ``out_dtype`` / ``memory_format`` outputs included) and each lookup is one
    autograd node that saves ``coords`` only.  Its backward makes one
    ``dxr_alt_corr_backward`` call per level with ``DXR_ALT_BWD_ACCUMULATE`` (the
    exact-f32 MFMA kernel of csrc/alt_corr_bwd.hip) on the NHWC fmap1, the level's
    pooled fmap2, ``coords / 2^l`` and the level's channel slice of ``grad_out``
    (one relayout pass per lookup) into zero-filled fmap-sized buffers, folds the
    level gradients of fmap2 down the pooling chain (level l gets level l+1's
    total / 4; the floor-mode remainder row / column gets 0), scales by
    1 / sqrt(D) and returns ``[B, D, H, W]`` gradients (permuted views); autograd
    sums the lookups.  Nothing proportional to (H*W)^2 is allocated and nothing
    but ``coords`` is held per lookup.

    bfloat16 / float16 fmaps that require grad are widened by an autograd-tracked
    ``.float()``, so their gradients arrive in the input dtype.  D % 16 != 0 or
    D > 256 (the library declines the flag, ``DXR_EUNSUPPORTED``) runs the
    unflagged per-query kernel and adds with torch: the same gradients to
    tolerance, except that that kernel returns NaN for a query with a NaN or
    infinite coordinate where the MFMA kernel drops it (exactly 0).  Fmaps and
    ``grad_out`` must be finite.  Coords that require grad raise
    ``NotImplementedError``, as everywhere; bad ``out_dtype`` / ``memory_format`` /
    ``volume_dtype`` raise ``ValueError`` before the native library is reached.
    ``volume_dtype=torch.float16`` with fmaps that require grad raises
    ``NotImplementedError`` before any launch, as ``CorrBlock``'s float16 pyramid
    does: a rounded forward with an exact backward is not offered silently.
    Without grad it behaves as the base class.
    """

    def __init__(self, fmap1, fmap2, num_levels=4, radius=4, *, out_dtype=None,
                 memory_format=None, **extensions):
        volume_dtype = _pop_volume_dtype(extensions)
        _out_flag(out_dtype)
        vol16 = _f16_volumes(volume_dtype)
        _layout_flag(memory_format)
        self._train = None
        self._bwd_native = True   # until the library declines the accumulate flag
        if isinstance(fmap1, torch.Tensor) and isinstance(fmap2, torch.Tensor) and \
                _wants_grad(fmap1, fmap2):
            _fmap_geometry(fmap1, fmap2)
            if vol16:
                # a rounded forward with an exact backward is not offered silently
                _require_no_grad(fmap1, fmap2,
                                 what="float16 coarse volumes (volume_dtype=torch.float16)")
            if fmap1.dtype in (torch.bfloat16, torch.float16):
                fmap1, fmap2 = fmap1.float(), fmap2.float()   # tracked: grads in the input dtype
            self._train = (fmap1, fmap2)
            fmap1, fmap2 = fmap1.detach(), fmap2.detach()
        super().__init__(fmap1, fmap2, num_levels, radius, out_dtype=out_dtype,
                         memory_format=memory_format, volume_dtype=volume_dtype)

    __init__.__signature__ = AlternateCorrBlock.__init__.__signature__

    def __call__(self, coords):
        if self._train is None or not torch.is_grad_enabled():
            return super().__call__(coords)
        B, D, H, W = self._geom
        _require_no_grad(coords, what="coords (the reference detaches them, core/raft.py:170)")
        c = _check_coords(coords, B, H, W, self._device)
        return _AltLookupGrad.apply(self._train[0], self._train[1], c, self)

    def _level_backward(self, lib, f2, c_l, g_l, f1g, f2g, flags):
        B, D, H, W = self._geom
        return lib.dxr_alt_corr_backward(self._f1_nhwc.data_ptr(), f2.data_ptr(), c_l.data_ptr(),
                                         g_l.data_ptr(), f1g.data_ptr(), f2g.data_ptr(), B, H, W,
                                         int(f2.shape[1]), int(f2.shape[2]), D, 1,
                                         self.radius | flags, nat.stream_of(f1g))

    def _lookup_backward(self, coords, gout, needs):
        """(dfmap1, dfmap2) of one lookup, ``[B, D, H, W]`` float32 views (None
        where not needed)."""
        B, D, H, W = self._geom
        L, rr = self.num_levels, (2 * self.radius + 1) ** 2
        dev = self._device
        # one relayout pass: [B, L*rr, H, W] of any dtype / memory format -> the L
        # contiguous float32 [B, 1, rr, H, W] slices the native call takes
        g = gout.reshape(B, L, rr, H, W).transpose(0, 1)
        if g.dtype != torch.float32 or not g.is_contiguous():
            g = torch.empty((L, B, rr, H, W), dtype=torch.float32, device=dev).copy_(g)
        # coords / 2^l as [B, 1, H, W, 2] per level (exact: powers of two)
        scale = torch.tensor([0.5 ** l for l in range(L)], dtype=torch.float32,
                             device=dev).view(L, 1, 1, 1, 1)
        cl = (coords.permute(0, 2, 3, 1).unsqueeze(0) * scale).contiguous()
        f1g = torch.zeros((B, H, W, D), dtype=torch.float32, device=dev)
        f2g = [torch.zeros_like(t) for t in self._f2_nhwc]
        lib = nat.load()
        what = "TrainableAlternateCorrBlock backward (dxr_alt_corr_backward)"
        with _Launch(dev):
            for l in range(L):
                if self._bwd_native:
                    st = self._level_backward(lib, self._f2_nhwc[l], cl[l], g[l], f1g, f2g[l],
                                              nat.DXR_ALT_BWD_ACCUMULATE)
                    if st == nat.DXR_EUNSUPPORTED and self.radius <= 6:
                        self._bwd_native = False   # remembered, as a declined output flag is
                    else:
                        nat.check(st, what)
                        continue
                # the library declined the flag (D % 16 != 0, D > 256): the per-query
                # kernel overwrites, torch adds
                t1 = torch.empty_like(f1g)
                nat.check(self._level_backward(lib, self._f2_nhwc[l], cl[l], g[l], t1, f2g[l], 0),
                          what)
                f1g += t1
        inv = 1.0 / _sqrt_dim(D)
        df1 = df2 = None
        if needs[0]:
            df1 = f1g.mul_(inv).permute(0, 3, 1, 2)
        if needs[1]:
            # avg_pool2d backward, coarse to fine: every covered cell gets a quarter
            tot = f2g[L - 1]
            for l in range(L - 2, -1, -1):
                q = tot * 0.25
                Ho, Wo = int(q.shape[1]), int(q.shape[2])
                fine = f2g[l][:, :2 * Ho, :2 * Wo]
                for a in range(2):
                    for b in range(2):
                        fine[:, a::2, b::2] += q
                tot = f2g[l]
            df2 = tot.mul_(inv).permute(0, 3, 1, 2)
        return df1, df2
