"""CPU: the output flags of the alternate block's lookups at the C-ABI and their
Python mapping.

DXR_OUT_F16 / DXR_OUT_BF16 / DXR_OUT_NHWC are or-ed onto the ``radius`` argument
of ``dxr_alt_corr_lookup``, ``dxr_alt_corr_lookup_ws``,
``dxr_alt_corr_lookup_levels_ws`` and ``dxr_alt_volume_lookup`` (the low byte is
the radius); the set of entry points and the ABI version do not change.  Every
call here is answered by an argument check before any launch (null pointers, an
empty batch, or a request the VALU forms decline), as in tests/test_capi.py, so
the file is safe without a GPU.
"""
from __future__ import annotations

import ctypes
import re
import subprocess

import pytest

from conftest import REPO

DECL = re.compile(r"^\s*(?:int|int64_t|const char\*)\s+(dxr_\w+)\s*\(", re.M)
P = 1 << 12   # a non-null, aligned dummy address: never dereferenced on these paths
F16, BF16, NHWC = 0x100, 0x200, 0x1000
VALID = (F16, BF16, NHWC, NHWC | F16, NHWC | BF16)
INVALID = (F16 | BF16, NHWC | F16 | BF16, 0x400, 0x800, 0x2000, 0x10000, NHWC | 0x400,
           F16 | 0x4000, 1 << 30)
ENTRIES = ("lookup", "lookup_ws", "levels_ws", "volume")


@pytest.fixture(scope="module")
def nat():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "_dxr_build_alt_out", REPO / "optical-flow_dexi-raft_amd" / "build.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build()  # no-op when fresh
    from dexiraft_amd import _native
    _native.load()
    return _native


def _call(nat, entry, radius, B=1, C=64, null=False, out=P):
    """One of the four entry points on a 16 x 16 map with 4 levels."""
    lib = nat.load()
    p = None if null else P
    o = None if null else out
    ptrs = None if null else (ctypes.c_void_p * 4)(P, P, P, P)
    if entry == "lookup":
        return lib.dxr_alt_corr_lookup(p, ptrs, p, o, B, 16, 16, C, 4, radius, 8.0, None)
    if entry == "lookup_ws":
        return lib.dxr_alt_corr_lookup_ws(p, ptrs, p, o, B, 16, 16, C, 4, radius, 8.0, p, 1 << 24,
                                          None)
    if entry == "levels_ws":
        return lib.dxr_alt_corr_lookup_levels_ws(p, ptrs, p, o, B, 16, 16, C, 4, 2, radius, 8.0, p,
                                                 1 << 24, None)
    assert entry == "volume"
    return lib.dxr_alt_volume_lookup(p, p, o, B, 16, 16, 4, 2, radius, 8.0, None)


def test_abi_and_entry_points_unchanged(nat):
    assert nat.load().dxr_abi_version() == nat.ABI_VERSION == 10
    header = (REPO / "include" / "dexiraft_corr.h").read_text()
    assert "#define DXR_ABI_VERSION 10" in header
    assert set(nat.SIGNATURES) == set(DECL.findall(header))
    out = subprocess.run(["nm", "-D", "--defined-only", str(nat.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()[-1].startswith("dxr_")}
    assert exported == set(nat.SIGNATURES)
    assert (nat.DXR_OUT_F16, nat.DXR_OUT_BF16, nat.DXR_OUT_NHWC) == (F16, BF16, NHWC)


def test_header_documents_the_flags_on_radius():
    header = (REPO / "include" / "dexiraft_corr.h").read_text()
    flat = " ".join(header.replace("*", " ").split())
    assert "Output flags on radius" in flat
    assert "the low byte is the radius" in flat
    for name in ("dxr_alt_corr_lookup_ws", "dxr_alt_corr_lookup_levels_ws", "dxr_alt_volume_lookup"):
        assert name in flat.split("Output flags on radius.")[1].split("int dxr_alt_corr_lookup(")[0]
    assert "DXR_EUNSUPPORTED" in flat.split("Which forms implement the flags")[1][:900]


@pytest.mark.parametrize("entry", ENTRIES)
def test_invalid_flag_combinations_are_einval_before_anything_else(nat, entry):
    """With null pointers, and with B = 0 (which an unflagged call answers with
    DXR_OK before it looks at the pointers): nothing can launch."""
    for hi in INVALID:
        for r in (0, 4, 6):
            assert _call(nat, entry, hi | r, B=0, null=True) == nat.DXR_EINVAL, hex(hi | r)
            assert _call(nat, entry, hi | r, B=1, null=True) == nat.DXR_EINVAL
            assert _call(nat, entry, hi | r, B=0) == nat.DXR_EINVAL
    # the unflagged answers they pre-empt
    assert _call(nat, entry, 4, B=0, null=True) == nat.DXR_OK
    assert _call(nat, entry, 4, B=1, null=True) == nat.DXR_EINVAL
    assert _call(nat, entry, -1, B=0) == nat.DXR_EINVAL
    assert _call(nat, entry, 9, B=0) == nat.DXR_EUNSUPPORTED


@pytest.mark.parametrize("entry", ENTRIES)
def test_valid_flags_pass_the_checks(nat, entry):
    """Empty batch: every check up to the launch passes and nothing is launched;
    without the feature a flagged radius is > 8 and DXR_EUNSUPPORTED."""
    for hi in VALID:
        assert _call(nat, entry, hi | 4, B=0) == nat.DXR_OK, hex(hi)
        assert _call(nat, entry, hi | 4, B=0, null=True) == nat.DXR_OK
        assert _call(nat, entry, hi | 4, B=1, null=True) == nat.DXR_EINVAL     # pointer checks
        # the radius proper is the low byte, with its own limits
        limit = 8 if entry == "volume" else 6
        assert _call(nat, entry, hi | (limit + 1), B=0) == nat.DXR_EUNSUPPORTED
        assert _call(nat, entry, hi | limit, B=0) == nat.DXR_OK
    # 16-bit elements need 2-byte alignment; float32 ones are not checked on the host
    for hi in (F16, BF16, NHWC | F16):
        assert _call(nat, entry, hi | 4, B=0, out=P + 1) == nat.DXR_EINVAL
        assert _call(nat, entry, hi | 4, B=0, out=P + 2) == nat.DXR_OK
    assert _call(nat, entry, NHWC | 4, B=0, out=P + 1) == nat.DXR_OK


@pytest.mark.parametrize("entry", ENTRIES[:3])
def test_valu_forms_decline_the_flags_without_a_launch(nat, entry):
    """C % 16 != 0 or C > 256: the per-query VALU forms, which the header says
    answer a flagged request with DXR_EUNSUPPORTED (the addresses are dummies: a
    launch would fault)."""
    for C in (36, 37, 272):
        for hi in VALID:
            assert _call(nat, entry, hi | 4, B=1, C=C) == nat.DXR_EUNSUPPORTED, (C, hex(hi))


def test_alt_corr_forward_takes_no_flags(nat):
    lib = nat.load()
    for hi in VALID:
        assert lib.dxr_alt_corr_forward(P, P, P, P, 0, 8, 8, 8, 8, 64, 1, hi | 4,
                                        None) == nat.DXR_EUNSUPPORTED   # a radius > 6, as before


def test_constructor_arguments_are_checked_before_the_library(monkeypatch):
    import inspect

    import torch

    import dexiraft_amd as dx
    from dexiraft_amd import _native as nat

    def no_launch(*a, **k):
        raise AssertionError("the native library was reached")

    monkeypatch.setattr(nat, "load", no_launch)
    f = torch.zeros(1, 16, 16, 16)
    for bad in (torch.float64, torch.int8, "float16", 16):
        with pytest.raises(ValueError, match="out_dtype"):
            dx.AlternateCorrBlock(f, f, out_dtype=bad)
    for bad in (torch.channels_last_3d, torch.preserve_format, "channels_last", 2):
        with pytest.raises(ValueError, match="channels_last"):
            dx.AlternateCorrBlock(f, f, memory_format=bad)
        with pytest.raises(ValueError, match="channels_last"):
            dx.AlternateCorrBlock(f, f, 4, 4, out_dtype=torch.float16, memory_format=bad)
    # the declared surface stays the reference's
    assert list(inspect.signature(dx.AlternateCorrBlock.__init__).parameters) == \
        ["self", "fmap1", "fmap2", "num_levels", "radius"]
    assert list(inspect.signature(dx.AlternateCorrBlock.__call__).parameters) == ["self", "coords"]
    # the two options are keyword-only, with default None
    init = dx.AlternateCorrBlock.__init__
    assert init.__code__.co_varnames[:init.__code__.co_argcount] == \
        ("self", "fmap1", "fmap2", "num_levels", "radius")
    assert init.__defaults__ == (4, 4)
    assert init.__kwdefaults__ == {"out_dtype": None, "memory_format": None}
