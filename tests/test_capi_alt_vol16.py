"""CPU: DXR_ALT_VOL_F16, the float16 cell type of the alternate block's coarse
volumes, at the C-ABI, and its Python mapping.

The flag is or-ed onto the ``first_level`` of ``dxr_alt_coarse_volumes`` /
``dxr_alt_coarse_volumes_ws`` (the low byte is the level: the volume GEMM stores
float16 cells) and onto the ``radius`` of ``dxr_alt_volume_lookup`` (which reads
them), alone or with the output flags; no entry point is added and the ABI
version stays.  Every call here is answered by an argument check before any
launch (the addresses are dummies: a launch would fault), so the file is safe
without a GPU.

The bit is 0x40000: 0x8000 and 0x20000 are the input flags, and 0x400, 0x800,
0x2000, 0x4000, 0x10000 and 1 << 30 are pinned as invalid by the C-ABI tests of
the other flags.  They stay unknown bits beside this flag too.  The entry
points that do not take it answer it as they answer the input flags: the three
on-the-fly lookups and the accumulating backward with DXR_EINVAL, the
reference FFI ``dxr_alt_corr_forward`` / ``_backward`` (no flags at all: any
high bit is just a radius > 6) with DXR_EUNSUPPORTED.
"""
from __future__ import annotations

import ctypes
import inspect
import re
import subprocess

import pytest

from conftest import REPO

DECL = re.compile(r"^\s*(?:int|int64_t|const char\*)\s+(dxr_\w+)\s*\(", re.M)
P = 1 << 12   # a non-null, 16-byte aligned dummy address: never dereferenced on these paths
VOL16, INBF, IN16 = 0x40000, 0x20000, 0x8000
F16, BF16, NHWC = 0x100, 0x200, 0x1000
OUT_FLAGS = (0, F16, BF16, NHWC, NHWC | F16, NHWC | BF16)
PINNED_INVALID = (0x400, 0x800, 0x2000, 0x4000, 0x10000, 1 << 30)


@pytest.fixture(scope="module")
def nat():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "_dxr_build_alt_vol16", REPO / "optical-flow_dexi-raft_amd" / "build.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build()  # no-op when fresh
    from dexiraft_amd import _native
    _native.load()
    return _native


def _lookup(nat, radius, B=1, vol=P, coords=P, out=P, L=4, first=2):
    return nat.load().dxr_alt_volume_lookup(vol, coords, out, B, 16, 16, L, first, radius, 8.0, None)


def _volumes(nat, ws, first, B=1, C=64, L=4, f1=P, levels=P, vol=P, H=64, W=64):
    """dxr_alt_coarse_volumes (ws False) or _ws on an H x W map with L levels."""
    lib = nat.load()
    ptrs = None if levels is None else (ctypes.c_void_p * 8)(*([levels] * 8))
    if ws:
        return lib.dxr_alt_coarse_volumes_ws(f1, ptrs, B, H, W, C, L, first, vol, P, 1 << 30, None)
    return lib.dxr_alt_coarse_volumes(f1, ptrs, B, H, W, C, L, first, vol, None)


def test_flag_is_declared_and_the_abi_is_unchanged(nat):
    header = (REPO / "include" / "dexiraft_corr.h").read_text()
    assert re.search(r"^#define DXR_ALT_VOL_F16 0x40000$", header, re.M)
    assert nat.DXR_ALT_VOL_F16 == VOL16
    assert nat.load().dxr_abi_version() == nat.ABI_VERSION == 10
    assert "#define DXR_ABI_VERSION 10" in header
    assert set(nat.SIGNATURES) == set(DECL.findall(header))
    out = subprocess.run(["nm", "-D", "--defined-only", str(nat.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()[-1].startswith("dxr_")}
    assert exported == set(nat.SIGNATURES)
    flat = " ".join(header.replace("*", " ").split())
    doc = flat.split("Float16 volumes.")[1].split("int64_t dxr_alt_volume_numel(")[0]
    for word in ("DXR_ALT_VOL_F16", "dxr_alt_coarse_volumes", "dxr_alt_coarse_volumes_ws",
                 "dxr_alt_volume_lookup", "C % 32 == 0", "DXR_EUNSUPPORTED", "DXR_EINVAL",
                 "16-byte aligned", "nearest even", "65504", "subnormals"):
        assert word in doc, word


def test_flagged_volume_lookups_are_answered_on_the_host(nat):
    """Without the feature the bit is an unknown flag: DXR_EINVAL for all of
    these."""
    EINVAL, EUNSUP, OK = nat.DXR_EINVAL, nat.DXR_EUNSUPPORTED, nat.DXR_OK
    for hi in OUT_FLAGS:
        f = VOL16 | hi
        for r in range(9):
            assert _lookup(nat, f | r, B=0) == OK, (hex(hi), r)
        assert _lookup(nat, f | 4, B=0, vol=None, coords=None, out=None) == OK
        assert _lookup(nat, f | 4, vol=None) == EINVAL
        assert _lookup(nat, f | 4, coords=None) == EINVAL
        assert _lookup(nat, f | 4, out=None) == EINVAL
        for r in (9, 255):   # the radius proper is the low byte, with its own limit
            assert _lookup(nat, f | r) == EUNSUP, r
            assert _lookup(nat, f | r, B=0) == EUNSUP, r
        assert _lookup(nat, f | 4, first=4) == EINVAL
        # an unknown bit or an input flag beside it: DXR_EINVAL before anything else
        for bad in PINNED_INVALID + (IN16, INBF, IN16 | INBF):
            for B in (0, 1):
                assert _lookup(nat, f | bad | 4, B=B) == EINVAL, (hex(hi), hex(bad))
    for bad in (F16 | BF16, NHWC | F16 | BF16):
        assert _lookup(nat, VOL16 | bad | 4, B=0) == EINVAL
    # 16-bit outputs need 2-byte alignment with the flag as without it
    assert _lookup(nat, VOL16 | F16 | 4, B=0, out=P + 1) == EINVAL
    assert _lookup(nat, VOL16 | F16 | 4, B=0, out=P + 2) == OK
    # as before without the flag; a negative radius's bit is no flag
    assert _lookup(nat, 4, B=0) == OK and _lookup(nat, 9, B=0) == EUNSUP
    for bad in (IN16, INBF) + PINNED_INVALID:
        assert _lookup(nat, bad | 4, B=0) == EINVAL
    for r in (-1, -VOL16, -(1 << 30)):
        assert _lookup(nat, r, B=0) == EINVAL
    assert nat.load().dxr_last_hip_error() == 0


@pytest.mark.parametrize("ws", [False, True], ids=["volumes", "volumes_ws"])
def test_flagged_volume_builds_are_answered_on_the_host(nat, ws):
    EINVAL, EUNSUP, OK = nat.DXR_EINVAL, nat.DXR_EUNSUPPORTED, nat.DXR_OK
    for first in range(4):
        assert _volumes(nat, ws, VOL16 | first, B=0) == OK, first
    assert _volumes(nat, ws, VOL16 | 2, B=0, f1=None, levels=None, vol=None) == OK
    for C in (32, 96, 256):
        assert _volumes(nat, ws, VOL16 | 2, B=0, C=C) == OK, C
    # the level proper is the low byte
    for first in (4, 5, 255):
        assert _volumes(nat, ws, VOL16 | first) == EINVAL, first
        assert _volumes(nat, ws, VOL16 | first, B=0) == EINVAL, first
    # any other high bit leaves a level beyond the last
    for bad in PINNED_INVALID + (IN16, INBF, F16, NHWC):
        assert _volumes(nat, ws, VOL16 | bad | 2, B=0) == EINVAL, hex(bad)
        assert _volumes(nat, ws, bad | 2, B=0) == EINVAL, hex(bad)
    assert _volumes(nat, ws, -VOL16, B=0) == EINVAL
    # null pointers, and float16 volumes off 16-byte alignment
    assert _volumes(nat, ws, VOL16 | 2, f1=None) == EINVAL
    assert _volumes(nat, ws, VOL16 | 2, levels=None) == EINVAL
    assert _volumes(nat, ws, VOL16 | 2, vol=None) == EINVAL
    for off in (2, 4, 8):
        assert _volumes(nat, ws, VOL16 | 2, vol=P + off) == EINVAL, off
    # valid requests the volume GEMM's float16 stores do not serve: declined, nothing launched
    for C in (48, 16, 80):   # C % 32 != 0: those levels take the FULL box form
        assert _volumes(nat, ws, VOL16 | 2, C=C) == EUNSUP, C
    assert _volumes(nat, ws, VOL16 | 2, L=5) == EUNSUP   # level 4 is row-major
    assert _volumes(nat, ws, VOL16 | 4, L=5) == EUNSUP
    for C in (40, 272):   # as without the flag
        assert _volumes(nat, ws, VOL16 | 2, C=C) == EUNSUP, C
        assert _volumes(nat, ws, 2, C=C) == EUNSUP, C
    # unflagged requests as before
    assert _volumes(nat, ws, 2, B=0) == OK and _volumes(nat, ws, 2, B=0, C=48) == OK
    assert _volumes(nat, ws, 2, B=0, L=5) == OK and _volumes(nat, ws, 4, B=0) == EINVAL
    # the element counts do not take the bit
    lib = nat.load()
    assert lib.dxr_alt_volume_numel(1, 64, 64, 4, 2) > 0
    assert lib.dxr_alt_volume_numel(1, 64, 64, 4, VOL16 | 2) == -1
    assert lib.dxr_alt_coarse_volumes_ws_bytes(1, 64, 64, 64, 4, VOL16 | 2) == -1
    assert lib.dxr_last_hip_error() == 0


def test_other_entry_points_do_not_take_the_flag(nat):
    EINVAL, EUNSUP = nat.DXR_EINVAL, nat.DXR_EUNSUPPORTED
    lib = nat.load()
    ptrs = (ctypes.c_void_p * 4)(P, P, P, P)
    for hi in (0, F16, NHWC, IN16, INBF):
        r = VOL16 | hi | 4
        for B in (0, 1):
            assert lib.dxr_alt_corr_lookup(P, ptrs, P, P, B, 16, 16, 64, 4, r, 8.0, None) == EINVAL
            assert lib.dxr_alt_corr_lookup_ws(P, ptrs, P, P, B, 16, 16, 64, 4, r, 8.0, P, 1 << 24,
                                              None) == EINVAL
            assert lib.dxr_alt_corr_lookup_levels_ws(P, ptrs, P, P, B, 16, 16, 64, 4, 2, r, 8.0, P,
                                                     1 << 24, None) == EINVAL
    for B in (0, 1):
        # the accumulating backward: an unknown bit
        assert lib.dxr_alt_corr_backward(P, P, P, P, P, P, B, 8, 8, 8, 8, 64, 1,
                                         nat.DXR_ALT_BWD_ACCUMULATE | VOL16 | 4, None) == EINVAL
        # the reference FFI is float-only and takes no flags: just a radius > 6
        assert lib.dxr_alt_corr_forward(P, P, P, P, B, 8, 8, 8, 8, 64, 1, VOL16 | 4, None) == EUNSUP
        assert lib.dxr_alt_corr_backward(P, P, P, P, P, P, B, 8, 8, 8, 8, 64, 1, VOL16 | 4,
                                         None) == EUNSUP
    assert lib.dxr_last_hip_error() == 0


def test_volume_dtype_is_checked_before_anything_else_and_the_signatures_stay():
    import torch

    import dexiraft_amd as dx

    cpu = torch.zeros(1, 64, 16, 16)
    for cls in (dx.AlternateCorrBlock, dx.TrainableAlternateCorrBlock):
        for bad in (torch.bfloat16, "float16", torch.int8, torch.float64, 16):
            with pytest.raises(ValueError, match="volume_dtype"):
                cls(cpu, cpu, volume_dtype=bad)
            with pytest.raises(ValueError, match="volume_dtype"):
                cls(None, None, volume_dtype=bad)   # before the fmaps are looked at
        # a valid value gets as far as the fmaps: host tensors are refused as ever
        for ok in (None, torch.float32, torch.float16):
            with pytest.raises(RuntimeError):
                cls(cpu, cpu, volume_dtype=ok)
        # out_dtype is still looked at first, and unknown keywords are a TypeError
        with pytest.raises(ValueError, match="out_dtype"):
            cls(cpu, cpu, out_dtype=torch.int8, volume_dtype=torch.int8)
        with pytest.raises(TypeError, match="volume_dtypes"):
            cls(cpu, cpu, volume_dtypes=torch.float16)
        assert list(inspect.signature(cls.__init__).parameters) == \
            ["self", "fmap1", "fmap2", "num_levels", "radius"]
        assert list(inspect.signature(cls.__call__).parameters) == ["self", "coords"]
        assert cls.__init__.__defaults__ == (4, 4)
        assert isinstance(cls.volume_dtype, property) and cls.volume_dtype.fset is None
