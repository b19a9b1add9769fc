"""ctypes binding of libdexiraft_corr.so (C-ABI: include/dexiraft_corr.h).

The shared object is loaded only after ``import torch`` so that its
``libamdhip64.so.7`` dependency resolves to the HIP runtime torch already
loaded: device pointers and streams are then shared with torch's allocator.
There is no fallback: if the library is missing or a call fails, an exception
is raised.
"""
from __future__ import annotations

import ctypes
import threading
from pathlib import Path

import torch  # noqa: F401  (must precede the CDLL load, see module docstring)

LIB_PATH = Path(__file__).resolve().with_name("libdexiraft_corr.so")
ABI_VERSION = 10

DXR_OK, DXR_EINVAL, DXR_EUNSUPPORTED, DXR_EHIP = 0, 1, 2, -1
DXR_F32, DXR_BF16, DXR_F16 = 0, 1, 2   # DXR_F16: an in_dtype of the pyramid builds only
DXR_PYR_F16 = 4   # float16 pyramid storage: a pyr_dtype only (build, unpack / pack, the lookups)
# output dtype flags, or-ed onto the pyr_dtype of dxr_corr_lookup / dxr_corr_lookup_conv1x1 and
# onto the radius of the alternate block's lookups (dxr_alt_corr_lookup, _ws, _levels_ws,
# dxr_alt_volume_lookup: the low byte is the radius)
DXR_OUT_F16, DXR_OUT_BF16 = 0x100, 0x200
# output layout flag of the same calls: `out` is [B, H, W, C] (channels-last); alone or with
# one dtype flag
DXR_OUT_NHWC = 0x1000
# accumulate flag of dxr_alt_corr_backward, or-ed onto its radius: the MFMA kernel adds the
# gradients into fmap1_grad / fmap2_grad (no memset; the caller zero-fills)
DXR_ALT_BWD_ACCUMULATE = 0x2000
# input dtype flag of dxr_alt_corr_lookup / _ws / _levels_ws, or-ed onto their radius (with or
# without output flags): fmap1 and fmap2 level 0 are float16, the pooled levels float32
DXR_ALT_IN_F16 = 0x8000
# the same for bfloat16 fmaps (one input flag at a time)
DXR_ALT_IN_BF16 = 0x20000
# float16 coarse volumes: or-ed onto the first_level of dxr_alt_coarse_volumes / _ws (the GEMM
# stores float16 cells) and onto the radius of dxr_alt_volume_lookup (which reads them)
DXR_ALT_VOL_F16 = 0x40000
DXR_NCHW, DXR_NHWC = 0, 1
DXR_BUILD_AUTO, DXR_BUILD_EXACT_F32 = 0, 1

# Every symbol include/dexiraft_corr.h declares, with its ctypes signature.
_i64 = ctypes.c_int64
_int = ctypes.c_int
_vp = ctypes.c_void_p
_f32 = ctypes.c_float
SIGNATURES: dict[str, tuple[object, list[object]]] = {
    "dxr_abi_version": (_int, []),
    "dxr_status_string": (ctypes.c_char_p, [_int]),
    "dxr_last_hip_error": (_int, []),
    "dxr_pyramid_numel": (_i64, [_i64, _i64, _i64, _int]),
    "dxr_pyramid_level_offset": (_i64, [_i64, _i64, _i64, _int]),
    "dxr_corr_pyramid_build": (_int, [_vp, _vp, _int, _int, _i64, _i64, _i64, _i64, _int, _f32,
                                      _vp, _int, _int, _vp]),
    "dxr_build_workspace_bytes": (_i64, [_int, _i64, _i64, _i64, _i64]),
    "dxr_corr_pyramid_build_ws": (_int, [_vp, _vp, _int, _int, _i64, _i64, _i64, _i64, _int,
                                         _f32, _vp, _int, _int, _vp, _i64, _vp]),
    "dxr_corr_volume": (_int, [_vp, _vp, _int, _i64, _i64, _i64, _i64, _f32, _vp, _vp]),
    "dxr_pyramid_unpack": (_int, [_vp, _int, _i64, _i64, _i64, _int, _int, _vp, _vp]),
    "dxr_pyramid_pack": (_int, [_vp, _i64, _i64, _i64, _int, _int, _vp, _int, _vp]),
    "dxr_corr_lookup": (_int, [_vp, _int, _i64, _i64, _i64, _int, _int, _vp, _vp, _vp]),
    "dxr_avg_pool2x2": (_int, [_vp, _vp, _i64, _i64, _i64, _vp]),
    "dxr_corr_lookup_backward": (_int, [_vp, _vp, _i64, _i64, _i64, _int, _int, _vp, _int, _vp]),
    "dxr_corr_lookup_backward_multi": (_int, [ctypes.POINTER(_vp), ctypes.POINTER(_vp), _int, _i64,
                                              _i64, _i64, _int, _int, _vp, _int, _vp]),
    "dxr_lookup_backward_bound_slots": (_i64, [_i64, _i64, _i64, _int, _int]),
    "dxr_corr_lookup_backward_multi_bound": (_int, [ctypes.POINTER(_vp), ctypes.POINTER(_vp), _int,
                                                    _i64, _i64, _i64, _int, _int, _vp, _int, _vp,
                                                    _vp]),
    "dxr_pyramid_backward": (_int, [_vp, _int, _i64, _i64, _i64, _int, _f32, _vp, _vp]),
    "dxr_fmap_grads_workspace_bytes": (_i64, [_i64, _i64, _i64, _i64, _int]),
    "dxr_fmap_grads": (_int, [_vp, _int, _vp, _vp, _i64, _i64, _i64, _i64, _int, _f32, _vp, _vp,
                              _vp, _i64, _vp]),
    "dxr_fmap_grads_bounded_workspace_bytes": (_i64, [_i64, _i64, _i64, _i64, _int]),
    "dxr_fmap_grads_bounded": (_int, [_vp, _int, _vp, _vp, _i64, _i64, _i64, _i64, _int, _f32, _vp,
                                      _i64, _vp, _vp, _vp, _i64, _vp]),
    "dxr_alt_corr_forward": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64,
                                    _i64, _int, _vp]),
    "dxr_alt_corr_backward": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64,
                                     _i64, _i64, _i64, _int, _vp]),
    "dxr_conv1x1_packed_bytes": (_i64, [_i64, _i64]),
    "dxr_conv1x1_pack_weight": (_int, [_vp, _i64, _i64, _vp, _vp]),
    "dxr_corr_lookup_conv1x1": (_int, [_vp, _int, _i64, _i64, _i64, _int, _int, _vp, _vp, _vp,
                                       _i64, _int, _vp, _vp]),
    "dxr_transpose": (_int, [_vp, _vp, _int, _i64, _i64, _i64, _vp]),
    "dxr_avg_pool2x2_nhwc": (_int, [_vp, _vp, _i64, _i64, _i64, _i64, _vp]),
    "dxr_alt_corr_lookup": (_int, [_vp, ctypes.POINTER(_vp), _vp, _vp, _i64, _i64, _i64, _i64,
                                   _int, _int, _f32, _vp]),
    "dxr_alt_workspace_bytes": (_i64, [_i64, _i64, _i64, _int]),
    "dxr_alt_corr_lookup_ws": (_int, [_vp, ctypes.POINTER(_vp), _vp, _vp, _i64, _i64, _i64, _i64,
                                      _int, _int, _f32, _vp, _i64, _vp]),
    "dxr_alt_corr_lookup_levels_ws": (_int, [_vp, ctypes.POINTER(_vp), _vp, _vp, _i64, _i64, _i64,
                                             _i64, _int, _int, _int, _f32, _vp, _i64, _vp]),
    "dxr_alt_volume_numel": (_i64, [_i64, _i64, _i64, _int, _int]),
    "dxr_alt_coarse_volumes": (_int, [_vp, ctypes.POINTER(_vp), _i64, _i64, _i64, _i64, _int, _int,
                                      _vp, _vp]),
    "dxr_alt_coarse_volumes_ws_bytes": (_i64, [_i64, _i64, _i64, _i64, _int, _int]),
    "dxr_alt_coarse_volumes_ws": (_int, [_vp, ctypes.POINTER(_vp), _i64, _i64, _i64, _i64, _int,
                                         _int, _vp, _vp, _i64, _vp]),
    "dxr_alt_volume_lookup": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _int, _int, _int, _f32, _vp]),
}

# Every symbol include/dexiraft_flow.h declares (prefix dxf_, its own ABI version; the same
# shared object).
FLOW_ABI_VERSION = 1
FLOW_SIGNATURES: dict[str, tuple[object, list[object]]] = {
    "dxf_abi_version": (_int, []),
    "dxf_forward_interpolate_workspace_bytes": (_i64, [_i64, _i64, _i64]),
    "dxf_forward_interpolate": (_int, [_vp, _i64, _i64, _i64, _vp, _vp, _i64, _vp]),
}

# Every symbol include/dexiraft_upsample.h declares (prefix dxu_, its own ABI version; the same
# shared object).
UPSAMPLE_ABI_VERSION = 1
DXU_MASK_F32, DXU_MASK_F16, DXU_MASK_BF16 = 0, 1, 2   # enum dxu_mask_dtype
UPSAMPLE_SIGNATURES: dict[str, tuple[object, list[object]]] = {
    "dxu_abi_version": (_int, []),
    "dxu_convex_upsample": (_int, [_vp, _int, _vp, _i64, _i64, _i64, _vp, _vp]),
    "dxu_convex_upsample_backward_workspace_bytes": (_i64, [_i64, _i64, _i64]),
    "dxu_convex_upsample_backward": (_int, [_vp, _vp, _int, _vp, _i64, _i64, _i64, _vp, _vp, _vp,
                                            _i64, _vp]),
}

# Every symbol include/dexiraft_loss.h declares (prefix dxl_, its own ABI version; the same
# shared object).
LOSS_ABI_VERSION = 1
_f64 = ctypes.c_double
LOSS_SIGNATURES: dict[str, tuple[object, list[object]]] = {
    "dxl_abi_version": (_int, []),
    "dxl_sequence_loss_workspace_bytes": (_i64, [_i64, _i64, _i64, _i64]),
    "dxl_sequence_loss": (_int, [ctypes.POINTER(_vp), _i64, _vp, _vp, _i64, _i64, _i64, _f64, _f32,
                                 _vp, _vp, _vp, _vp, _i64, _vp]),
    "dxl_sequence_loss_backward": (_int, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _i64, _vp,
                                          _vp, _i64, _i64, _i64, _f64, _f32, _vp]),
}

# Every symbol include/dexiraft_gru.h declares (prefix dxg_, its own ABI version), in a
# shared object of their own, libdexiraft_gru.so, which depends on libdexiraft_corr.so.
GRU_LIB_PATH = LIB_PATH.with_name("libdexiraft_gru.so")
GRU_ABI_VERSION = 1
DXG_F32, DXG_F16, DXG_BF16 = 0, 1, 2   # enum dxg_dtype
_g5 = [_i64, _i64, _i64, _i64, _i64]   # N, H, W, Ch, Cx
GRU_SIGNATURES: dict[str, tuple[object, list[object]]] = {
    "dxg_abi_version": (_int, []),
    "dxg_sepconv_packed_weight_bytes": (_i64, [_i64, _i64]),
    "dxg_sepconv_pack_weights": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _int, _vp, _i64,
                                        _vp]),
    "dxg_sepconv_workspace_bytes": (_i64, _g5),
    "dxg_sepconv_pack_inputs": (_int, [_vp, _int, _vp, _int, *_g5, _int, _vp, _i64, _vp]),
    "dxg_sepconv_gate_zr": (_int, [_vp, _int, *_g5, _int, _vp, _i64, _vp]),
    "dxg_sepconv_gate_qh": (_int, [_vp, _int, *_g5, _int, _vp, _int, _vp, _i64, _vp]),
    "dxg_sepconv_gru": (_int, [_vp, _int, _vp, _int, _vp, _vp, *_g5, _int, _vp, _int, _vp, _i64,
                               _vp]),
}

_lock = threading.Lock()
_lib: ctypes.CDLL | None = None
_gru_lib: ctypes.CDLL | None = None


def load() -> ctypes.CDLL:
    """Load (once) and return the native library; raise if it is unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not LIB_PATH.exists():
                raise ImportError(
                    f"{LIB_PATH.name} not found next to {Path(__file__).name}; build it with "
                    "`python optical-flow_dexi-raft_amd/build.py` (hipcc, gfx950)")
            lib = ctypes.CDLL(str(LIB_PATH))
            for name, (res, args) in (*SIGNATURES.items(), *FLOW_SIGNATURES.items(),
                                            *UPSAMPLE_SIGNATURES.items(),
                                            *LOSS_SIGNATURES.items()):
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
            ver = lib.dxr_abi_version()
            if ver != ABI_VERSION:
                raise ImportError(f"{LIB_PATH.name} ABI {ver} != expected {ABI_VERSION}; rebuild")
            ver = lib.dxf_abi_version()
            if ver != FLOW_ABI_VERSION:
                raise ImportError(f"{LIB_PATH.name} flow ABI {ver} != expected {FLOW_ABI_VERSION}; "
                                  "rebuild")
            ver = lib.dxu_abi_version()
            if ver != UPSAMPLE_ABI_VERSION:
                raise ImportError(f"{LIB_PATH.name} upsample ABI {ver} != expected "
                                  f"{UPSAMPLE_ABI_VERSION}; rebuild")
            ver = lib.dxl_abi_version()
            if ver != LOSS_ABI_VERSION:
                raise ImportError(f"{LIB_PATH.name} loss ABI {ver} != expected {LOSS_ABI_VERSION}; "
                                  "rebuild")
            _lib = lib
    return _lib


def load_gru() -> ctypes.CDLL:
    """Load (once) and return libdexiraft_gru.so, after the library it depends on."""
    global _gru_lib
    if _gru_lib is not None:
        return _gru_lib
    load()
    with _lock:
        if _gru_lib is None:
            if not GRU_LIB_PATH.exists():
                raise ImportError(
                    f"{GRU_LIB_PATH.name} not found next to {Path(__file__).name}; build it with "
                    "`python optical-flow_dexi-raft_amd/build.py` (hipcc, gfx950)")
            lib = ctypes.CDLL(str(GRU_LIB_PATH))
            for name, (res, args) in GRU_SIGNATURES.items():
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
            ver = lib.dxg_abi_version()
            if ver != GRU_ABI_VERSION:
                raise ImportError(f"{GRU_LIB_PATH.name} ABI {ver} != expected {GRU_ABI_VERSION}; "
                                  "rebuild")
            _gru_lib = lib
    return _gru_lib


def check(status: int, what: str) -> None:
    """Raise the exception the reference would raise for a failed call."""
    if status == DXR_OK:
        return
    lib = load()
    msg = lib.dxr_status_string(status).decode()
    if status == DXR_EHIP:
        raise RuntimeError(f"{what}: HIP error {lib.dxr_last_hip_error()} ({msg})")
    if status == DXR_EUNSUPPORTED:
        raise NotImplementedError(f"{what}: {msg}")
    raise RuntimeError(f"{what}: {msg}")


# torch's raw current-stream query: ~0.3 us per call against ~2 us for
# torch.cuda.current_stream(dev).cuda_stream, which builds a Stream object (the
# eager lookup path is host-bound: scripts/probe_host_overhead.py)
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_of(t: torch.Tensor) -> int:
    """hipStream_t (as int) of torch's current stream on t's device."""
    if _raw_stream is not None:
        return _raw_stream(t.device.index)
    return torch.cuda.current_stream(t.device).cuda_stream


def ptr(t: torch.Tensor | None) -> int | None:
    return None if t is None else t.data_ptr()
