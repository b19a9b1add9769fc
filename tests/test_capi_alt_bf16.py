"""CPU: DXR_ALT_IN_BF16, the bfloat16-fmaps flag of the alternate block's
on-the-fly lookups, at the C-ABI, and its Python mapping.

The flag is or-ed onto the ``radius`` of ``dxr_alt_corr_lookup``,
``dxr_alt_corr_lookup_ws`` and ``dxr_alt_corr_lookup_levels_ws`` (the low byte is
the radius), alone or with the output flags; no entry point is added and the ABI
version stays.  Every call here is answered by an argument check before any
launch (the addresses are dummies: a launch would fault), so the file is safe
without a GPU.

The bit is 0x20000: 0x8000 is ``DXR_ALT_IN_F16``, and 0x400, 0x800, 0x2000,
0x4000, 0x10000 and 1 << 30 are pinned as invalid by the C-ABI tests of the
output flags and of the float16 flag.  They stay unknown bits beside this flag
too (checked below), and the two input flags exclude each other.

The entry points that do not take the flag answer it as they answer
``DXR_ALT_IN_F16``: ``dxr_alt_volume_lookup`` and the accumulating
``dxr_alt_corr_backward`` with DXR_EINVAL (an unknown bit), and the reference
FFI ``dxr_alt_corr_forward`` / ``_backward`` — float-only, no flags at all, so
any high bit is just a radius > 6 — with DXR_EUNSUPPORTED, as
tests/test_capi_alt_f16.py pins for the float16 flag.
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
INBF, IN16 = 0x20000, 0x8000
F16, BF16, NHWC = 0x100, 0x200, 0x1000
OUT_FLAGS = (0, F16, BF16, NHWC, NHWC | F16, NHWC | BF16)
PINNED_INVALID = (0x400, 0x800, 0x2000, 0x4000, 0x10000, 1 << 30)
ENTRIES = ("lookup", "lookup_ws", "levels_ws")


@pytest.fixture(scope="module")
def nat():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "_dxr_build_alt_bf16", REPO / "optical-flow_dexi-raft_amd" / "build.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build()  # no-op when fresh
    from dexiraft_amd import _native
    _native.load()
    return _native


def _call(nat, entry, radius, B=1, C=64, f1=P, levels=(P, P, P, P), coords=P, out=P):
    """One of the three entry points on a 16 x 16 map with 4 levels."""
    lib = nat.load()
    ptrs = None if levels is None else (ctypes.c_void_p * 4)(*levels)
    if entry == "lookup":
        return lib.dxr_alt_corr_lookup(f1, ptrs, coords, out, B, 16, 16, C, 4, radius, 8.0, None)
    if entry == "lookup_ws":
        return lib.dxr_alt_corr_lookup_ws(f1, ptrs, coords, out, B, 16, 16, C, 4, radius, 8.0, P,
                                          1 << 24, None)
    assert entry == "levels_ws"
    return lib.dxr_alt_corr_lookup_levels_ws(f1, ptrs, coords, out, B, 16, 16, C, 4, 2, radius, 8.0,
                                             P, 1 << 24, None)


def test_flag_is_declared_and_the_abi_is_unchanged(nat):
    header = (REPO / "include" / "dexiraft_corr.h").read_text()
    assert re.search(r"^#define DXR_ALT_IN_BF16 0x20000$", header, re.M)
    assert re.search(r"^#define DXR_ALT_IN_F16 0x8000$", header, re.M)
    assert nat.DXR_ALT_IN_BF16 == INBF and nat.DXR_ALT_IN_F16 == IN16
    assert nat.load().dxr_abi_version() == nat.ABI_VERSION == 10
    assert "#define DXR_ABI_VERSION 10" in header
    assert set(nat.SIGNATURES) == set(DECL.findall(header))
    out = subprocess.run(["nm", "-D", "--defined-only", str(nat.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()[-1].startswith("dxr_")}
    assert exported == set(nat.SIGNATURES)
    flat = " ".join(header.replace("*", " ").split())
    doc = flat.split("Bfloat16 fmaps on radius.")[1].split("int dxr_alt_corr_lookup(")[0]
    for word in ("DXR_ALT_IN_BF16", "DXR_ALT_IN_F16", "dxr_alt_corr_lookup_ws",
                 "dxr_alt_corr_lookup_levels_ws", "core/raft.py:139-142", "C % 16 == 0", "C <= 256",
                 "16-byte aligned", "DXR_EUNSUPPORTED", "DXR_EINVAL", "float32"):
        assert word in doc, word


@pytest.mark.parametrize("entry", ENTRIES)
def test_flagged_requests_are_answered_on_the_host(nat, entry):
    """Without the feature the bit is an unknown flag: DXR_EINVAL for all of
    these."""
    EINVAL, EUNSUP, OK = nat.DXR_EINVAL, nat.DXR_EUNSUPPORTED, nat.DXR_OK
    for hi in OUT_FLAGS:
        f = INBF | hi
        # an empty batch: every check passes, nothing is launched
        for r in range(7):
            assert _call(nat, entry, f | r, B=0) == OK, (hex(hi), r)
        assert _call(nat, entry, f | 4, B=0, f1=None, levels=None, coords=None, out=None) == OK
        for C in (16, 32, 48, 80, 256):
            assert _call(nat, entry, f | 4, B=0, C=C) == OK, (hex(hi), C)
        # channel counts the MFMA form does not serve: declined, nothing launched
        for C in (40, 272, 36, 37, 8):
            assert _call(nat, entry, f | 4, C=C) == EUNSUP, (hex(hi), C)
        # the radius proper is the low byte, with its own limit
        for r in (7, 8, 255):
            assert _call(nat, entry, f | r) == EUNSUP, r
            assert _call(nat, entry, f | r, B=0) == EUNSUP, r
        # null pointers
        assert _call(nat, entry, f | 4, f1=None) == EINVAL
        assert _call(nat, entry, f | 4, levels=None) == EINVAL
        assert _call(nat, entry, f | 4, levels=(None, P, P, P)) == EINVAL
        assert _call(nat, entry, f | 4, levels=(P, None, P, P)) == EINVAL
        assert _call(nat, entry, f | 4, coords=None) == EINVAL
        assert _call(nat, entry, f | 4, out=None) == EINVAL
        # operands off 16-byte alignment: no bfloat16 form serves them
        assert _call(nat, entry, f | 4, f1=P + 8) == EUNSUP
        assert _call(nat, entry, f | 4, levels=(P + 8, P, P, P)) == EUNSUP
        assert _call(nat, entry, f | 4, levels=(P, P + 4, P, P)) == EUNSUP
        # one input dtype at a time: both flags are DXR_EINVAL before anything else
        for r in (0, 4, 6, 7):
            assert _call(nat, entry, f | IN16 | r, B=0) == EINVAL, (hex(hi), r)
            assert _call(nat, entry, f | IN16 | r) == EINVAL, (hex(hi), r)
            assert _call(nat, entry, f | IN16 | r, C=40) == EINVAL, (hex(hi), r)
    # an unknown high bit beside the flag, or both output dtypes: DXR_EINVAL before anything else
    for bad in PINNED_INVALID + (F16 | BF16, NHWC | F16 | BF16):
        for r in (0, 4, 6):
            assert _call(nat, entry, INBF | bad | r, B=0) == EINVAL, hex(bad)
            assert _call(nat, entry, INBF | bad | r, B=1, f1=None, levels=None) == EINVAL
    # 16-bit outputs need 2-byte alignment with the flag as without it
    assert _call(nat, entry, INBF | F16 | 4, B=0, out=P + 1) == EINVAL
    assert _call(nat, entry, INBF | F16 | 4, B=0, out=P + 2) == OK
    # geometry is checked as in the unflagged call
    assert _call(nat, entry, INBF | 4, B=-1) == EINVAL
    assert _call(nat, entry, INBF | 4, C=0) == EINVAL
    assert nat.load().dxr_last_hip_error() == 0


@pytest.mark.parametrize("entry", ENTRIES)
def test_other_requests_are_answered_as_before(nat, entry):
    EINVAL, EUNSUP, OK = nat.DXR_EINVAL, nat.DXR_EUNSUPPORTED, nat.DXR_OK
    assert _call(nat, entry, 4, B=0) == OK
    assert _call(nat, entry, 4, B=0, C=40) == OK
    assert _call(nat, entry, 9, B=0) == EUNSUP
    assert _call(nat, entry, 4, f1=None) == EINVAL
    for hi in OUT_FLAGS:
        assert _call(nat, entry, hi | 4, B=0) == OK
        assert _call(nat, entry, IN16 | hi | 4, B=0) == OK
        assert _call(nat, entry, IN16 | hi | 4, C=40) == EUNSUP
    # the flag bit of a negative radius (two's complement) is not a flag
    for r in (-1, -INBF, -(1 << 30)):
        assert _call(nat, entry, r, B=0) == EINVAL


def test_other_entry_points_do_not_take_the_flag(nat):
    """As they do not take DXR_ALT_IN_F16 (module docstring): the same status
    for either input flag."""
    EINVAL, EUNSUP = nat.DXR_EINVAL, nat.DXR_EUNSUPPORTED
    lib = nat.load()
    for hi in (0, F16, NHWC):
        for flag in (INBF, IN16):
            # dxr_alt_volume_lookup reads no fmaps: an unknown bit
            r = flag | hi | 4
            assert lib.dxr_alt_volume_lookup(P, P, P, 0, 16, 16, 4, 2, r, 8.0, None) == EINVAL
            assert lib.dxr_alt_volume_lookup(P, P, P, 1, 16, 16, 4, 2, r, 8.0, None) == EINVAL
            # the reference FFI is float-only and takes no flags: just a radius > 6
            assert lib.dxr_alt_corr_forward(P, P, P, P, 0, 8, 8, 8, 8, 64, 1, r, None) == EUNSUP
            assert lib.dxr_alt_corr_forward(P, P, P, P, 1, 8, 8, 8, 8, 64, 1, r, None) == EUNSUP
            assert lib.dxr_alt_corr_backward(P, P, P, P, P, P, 0, 8, 8, 8, 8, 64, 1, r,
                                             None) == EUNSUP
            assert lib.dxr_alt_corr_backward(P, P, P, P, P, P, 1, 8, 8, 8, 8, 64, 1, r,
                                             None) == EUNSUP
    # beside the accumulate flag it is an unknown bit
    for B in (0, 1):
        assert lib.dxr_alt_corr_backward(P, P, P, P, P, P, B, 8, 8, 8, 8, 64, 1,
                                         nat.DXR_ALT_BWD_ACCUMULATE | INBF | 4, None) == EINVAL
    # (dxr_alt_coarse_volumes* have no radius argument to carry a flag)
    assert nat.load().dxr_last_hip_error() == 0


def test_native_bf16_is_a_class_knob_and_the_signatures_stay():
    import dexiraft_amd as dx

    assert isinstance(dx.AlternateCorrBlock.NATIVE_BF16, bool)
    assert dx.TrainableAlternateCorrBlock.NATIVE_BF16 is dx.AlternateCorrBlock.NATIVE_BF16
    assert dx.AlternateCorrBlock.NATIVE_F16 is True
    for cls in (dx.AlternateCorrBlock, dx.TrainableAlternateCorrBlock):
        assert list(inspect.signature(cls.__init__).parameters) == \
            ["self", "fmap1", "fmap2", "num_levels", "radius"]
        assert list(inspect.signature(cls.__call__).parameters) == ["self", "coords"]
        init = cls.__init__
        assert init.__defaults__ == (4, 4)
        assert init.__kwdefaults__ == {"out_dtype": None, "memory_format": None}
