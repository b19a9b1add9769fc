"""``SepConvGRU``: the reference's separable GRU (core/update.py:33-60) as five HIP
launches on the matrix cores, for inference (include/dexiraft_gru.h, csrc/gru_sepconv.hip).

The six convolutions run on float16 or bfloat16 operands with float32
accumulation; the state stays float32 between the stages, so this form has fewer
roundings than the reference under ``torch.autocast``.  There is no float32 compute
dtype, no backward and no fallback: a shape the kernels do not take is a
``ValueError``.
"""
from __future__ import annotations

import torch

from . import _native

__all__ = ["SepConvGRU"]

_NAMES = ("convz1", "convr1", "convq1", "convz2", "convr2", "convq2")
_DXG = {torch.float32: _native.DXG_F32, torch.float16: _native.DXG_F16,
        torch.bfloat16: _native.DXG_BF16}


def check_channels(ch: int, cx: int) -> None:
    """ValueError unless the kernels take ``ch`` hidden and ``cx`` input channels."""
    if ch % 16 or not 16 <= ch <= 128 or cx % 16 or not 16 <= cx <= 256:
        raise ValueError(f"SepConvGRU: unsupported channels hidden={ch}, input={cx} "
                         "(hidden: a multiple of 16 in 16..128, input: a multiple of 16 in 16..256)")


def workspace_views(ws: torch.Tensor, N: int, H: int, W: int, ch: int, cx: int,
                    compute_dtype: torch.dtype) -> dict[str, torch.Tensor]:
    """The five channels-last tensors of a workspace (a uint8 tensor of at least
    ``dxg_sepconv_workspace_bytes``), as views: ``h32``, ``hc``, ``xc``, ``z``, ``rh``."""
    P, out, off = N * H * W, {}, 0
    for name, dt, c in (("h32", torch.float32, ch), ("hc", compute_dtype, ch),
                        ("xc", compute_dtype, cx), ("z", torch.float32, ch),
                        ("rh", compute_dtype, ch)):
        nbytes = P * c * (4 if dt == torch.float32 else 2)
        out[name] = ws[off:off + nbytes].view(dt).view(N, H, W, c)
        off += nbytes
    return out


class SepConvGRU:
    """Drop-in inference forward of the reference's ``SepConvGRU``: ``gru(h, x) -> h``.

    ``SepConvGRU(weights, compute_dtype=torch.bfloat16)`` takes a dict with the keys
    ``convz1.weight``, ``convz1.bias``, ... ``convq2.bias`` (a ``state_dict()`` of the
    reference module): the horizontal weights ``[Ch, Ch + Cx, 1, 5]``, the vertical
    ones ``[Ch, Ch + Cx, 5, 1]``, the biases ``[Ch]``.  ``SepConvGRU.from_module(m)``
    takes any module with ``convz1`` ... ``convq2`` of those shapes and follows its
    parameters: they are packed into MFMA operand order on the first call and again
    whenever one of them was modified in place (``Tensor._version``), replaced,
    given other storage (``param.data = ...``: ``data_ptr()``), or the device changes.
    A write that bypasses all three (through a ``.data`` view, say) is not seen:
    build a new ``SepConvGRU`` then.

    ``h``: ``[N, Ch, H, W]``, ``x``: ``[N, Cx, H, W]``, float32, float16 or bfloat16,
    on one HIP device; the result has ``h``'s dtype.  Everything runs on torch's
    current stream with a workspace from the caching allocator and without a
    synchronisation, so a call can sit inside a captured graph (call once before
    the capture, so that the weights are packed outside it).

    Inference only: with grad mode on, an input or weight that requires grad raises
    ``RuntimeError`` (call under ``torch.no_grad()``).  Non-finite inputs do not
    fault; what they produce is unspecified.
    """

    def __init__(self, weights, compute_dtype: torch.dtype = torch.bfloat16):
        if compute_dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(f"compute_dtype must be torch.float16 or torch.bfloat16, got "
                             f"{compute_dtype} (float32 compute is not implemented)")
        self.compute_dtype = compute_dtype
        self._source = weights if callable(weights) else (lambda: weights)
        params = self._params()
        w = params[0]
        if w.dim() != 4 or tuple(w.shape[2:]) != (1, 5) or w.shape[1] <= w.shape[0]:
            raise ValueError(f"convz1.weight must be [Ch, Ch + Cx, 1, 5], got {tuple(w.shape)}")
        ch, cx = int(w.shape[0]), int(w.shape[1] - w.shape[0])
        for i, name in enumerate(_NAMES):
            want = (ch, ch + cx, 1, 5) if i < 3 else (ch, ch + cx, 5, 1)
            if tuple(params[2 * i].shape) != want or tuple(params[2 * i + 1].shape) != (ch,):
                raise ValueError(f"{name}: weight {tuple(params[2 * i].shape)} / bias "
                                 f"{tuple(params[2 * i + 1].shape)}, expected {want} / {(ch,)}")
        check_channels(ch, cx)
        self.hidden_dim, self.input_dim = ch, cx
        self._packed = None     # (key, packed_h, packed_v)

    @classmethod
    def from_module(cls, module, compute_dtype: torch.dtype = torch.bfloat16) -> "SepConvGRU":
        for name in _NAMES:
            conv = getattr(module, name, None)
            if getattr(conv, "weight", None) is None or getattr(conv, "bias", None) is None:
                raise ValueError(f"from_module: the module has no {name} with a weight and a bias")
        return cls(lambda: {f"{n}.{k}": getattr(getattr(module, n), k)
                            for n in _NAMES for k in ("weight", "bias")}, compute_dtype)

    def _params(self) -> list[torch.Tensor]:
        d = self._source()
        try:
            params = [d[f"{n}.{k}"] for n in _NAMES for k in ("weight", "bias")]
        except (KeyError, TypeError) as e:
            raise ValueError(f"SepConvGRU: weights must map convz1.weight ... convq2.bias ({e})")
        for p in params:
            if not isinstance(p, torch.Tensor):
                raise TypeError(f"SepConvGRU: weights must be tensors, got {type(p).__name__}")
        return params

    def _pack(self, params, device) -> tuple[torch.Tensor, torch.Tensor]:
        key = (device, tuple((id(p), p._version, p.data_ptr()) for p in params))
        if self._packed is not None and self._packed[0] == key:
            return self._packed[1], self._packed[2]
        lib = _native.load_gru()
        ch, cx = self.hidden_dim, self.input_dim
        nbytes = lib.dxg_sepconv_packed_weight_bytes(ch, cx)
        packed = []
        with torch.cuda.device(device):
            for axis in range(2):
                t = [p.detach().to(device=device, dtype=torch.float32).contiguous()
                     for p in params[6 * axis:6 * axis + 6]]
                buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
                _native.check(lib.dxg_sepconv_pack_weights(
                    t[0].data_ptr(), t[2].data_ptr(), t[4].data_ptr(), t[1].data_ptr(),
                    t[3].data_ptr(), t[5].data_ptr(), ch, cx, _DXG[self.compute_dtype],
                    buf.data_ptr(), nbytes, _native.stream_of(buf)), "dxg_sepconv_pack_weights")
                packed.append(buf)
        self._packed = (key, packed[0], packed[1])
        return packed[0], packed[1]

    def __call__(self, h: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        for name, t in (("h", h), ("x", x)):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
            if t.dtype not in _DXG:
                raise TypeError(f"{name} must be float32, float16 or bfloat16, got {t.dtype}")
        ch, cx = self.hidden_dim, self.input_dim
        if h.dim() != 4 or h.shape[1] != ch:
            raise ValueError(f"h must be [N, {ch}, H, W], got {tuple(h.shape)}")
        if x.dim() != 4 or x.shape[1] != cx:
            raise ValueError(f"x must be [N, {cx}, H, W], got {tuple(x.shape)}")
        if (x.shape[0], *x.shape[2:]) != (h.shape[0], *h.shape[2:]):
            raise ValueError(f"h {tuple(h.shape)} and x {tuple(x.shape)} differ in N, H or W")
        if h.device != x.device:
            raise ValueError(f"h is on {h.device}, x on {x.device}")
        params = self._params()
        if torch.is_grad_enabled() and any(t.requires_grad for t in (h, x, *params)):
            raise RuntimeError(
                "SepConvGRU is an inference forward: no gradient flows through it, and an input "
                "or weight requires grad; call it under torch.no_grad() (training through the "
                "fused GRU is not implemented)")
        if not h.is_cuda:
            raise RuntimeError("SepConvGRU: h and x must be on a HIP device (no CPU path)")
        N, _, H, W = (int(s) for s in h.shape)
        if N > 65535 or H < 1 or W < 1 or H * W > 2 ** 22:
            raise ValueError(f"SepConvGRU: unsupported geometry N={N}, H={H}, W={W} "
                             "(N <= 65535, 1 <= H*W <= 2**22)")
        lib = _native.load_gru()
        packed_h, packed_v = self._pack(params, h.device)
        h, x = h.detach().contiguous(), x.detach().contiguous()
        with torch.cuda.device(h.device):
            out = torch.empty_like(h)
            if N == 0:
                return out
            nbytes = lib.dxg_sepconv_workspace_bytes(N, H, W, ch, cx)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=h.device)
            _native.check(lib.dxg_sepconv_gru(
                h.data_ptr(), _DXG[h.dtype], x.data_ptr(), _DXG[x.dtype], packed_h.data_ptr(),
                packed_v.data_ptr(), N, H, W, ch, cx, _DXG[self.compute_dtype], out.data_ptr(),
                _DXG[out.dtype], ws.data_ptr(), nbytes, _native.stream_of(h)), "dxg_sepconv_gru")
        return out

    forward = __call__
