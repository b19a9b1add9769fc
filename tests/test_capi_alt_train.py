"""CPU: the accumulate flag of ``dxr_alt_corr_backward`` at the C-ABI and the
Python surface of ``TrainableAlternateCorrBlock``.

``DXR_ALT_BWD_ACCUMULATE`` (0x2000) is or-ed onto the ``radius`` argument (the low
byte is the radius); the set of entry points and the ABI version do not change.
Every call here is answered by an argument check before any launch (the
addresses are dummies: a launch would fault), so the file is safe without a GPU.
"""
from __future__ import annotations

import inspect
import re
import subprocess

import pytest

from conftest import REPO

DECL = re.compile(r"^\s*(?:int|int64_t|const char\*)\s+(dxr_\w+)\s*\(", re.M)
P = 1 << 12   # a non-null, 16-byte aligned dummy address: never dereferenced on these paths
ACC = 0x2000


@pytest.fixture(scope="module")
def nat():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "_dxr_build_alt_train", REPO / "optical-flow_dexi-raft_amd" / "build.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build()  # no-op when fresh
    from dexiraft_amd import _native
    _native.load()
    return _native


def _call(nat, radius, B=1, C=64, Nc=1, ptrs=(P, P, P, P, P, P)):
    """dxr_alt_corr_backward on 8 x 8 maps."""
    return nat.load().dxr_alt_corr_backward(*ptrs, B, 8, 8, 8, 8, C, Nc, radius, None)


def test_header_defines_the_flag_and_the_entry_points_are_unchanged(nat):
    header = (REPO / "include" / "dexiraft_corr.h").read_text()
    assert "#define DXR_ALT_BWD_ACCUMULATE 0x2000" in header
    assert nat.DXR_ALT_BWD_ACCUMULATE == ACC
    assert "#define DXR_ABI_VERSION 10" in header
    assert nat.load().dxr_abi_version() == nat.ABI_VERSION == 10
    assert set(nat.SIGNATURES) == set(DECL.findall(header))
    out = subprocess.run(["nm", "-D", "--defined-only", str(nat.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()[-1].startswith("dxr_")}
    assert exported == set(nat.SIGNATURES)
    # documented where the entry point is declared
    flat = " ".join(header.replace("*", " ").split())
    doc = flat.split("Stage (d), reference-FFI backward")[1].split("int dxr_alt_corr_backward(")[0]
    for word in ("DXR_ALT_BWD_ACCUMULATE", "ADDED INTO", "zero-fills", "DXR_EUNSUPPORTED",
                 "DXR_EINVAL", "finite", "C % 16 == 0", "C <= 256", "16-byte aligned"):
        assert word in doc, word


def test_flagged_validation_is_answered_on_the_host(nat):
    EINVAL, EUNSUP, OK = nat.DXR_EINVAL, nat.DXR_EUNSUPPORTED, nat.DXR_OK
    lib = nat.load()
    # null pointers
    for i in range(6):
        ptrs = tuple(None if k == i else P for k in range(6))
        assert _call(nat, ACC | 4, ptrs=ptrs) == EINVAL, i
    assert _call(nat, ACC | 4, ptrs=(None,) * 6) == EINVAL
    # any other bit above the low byte
    for hi in (0x100, 0x200, 0x400, 0x800, 0x1000, 0x4000, 0x10000, 1 << 30):
        assert _call(nat, ACC | hi | 4) == EINVAL, hex(hi)
        assert _call(nat, ACC | hi | 4, B=0) == EINVAL
        assert _call(nat, ACC | hi | 4, C=36) == EINVAL
    # shapes the MFMA kernel does not serve: declined, nothing launched
    for C in (36, 37, 8, 272, 512):
        assert _call(nat, ACC | 4, C=C) == EUNSUP, C
    for r in (7, 8, 255):
        assert _call(nat, ACC | r) == EUNSUP, r
        assert _call(nat, ACC | r, B=0) == EUNSUP
    for i in (0, 1, 4, 5):      # a fmap or gradient pointer 4 bytes off 16-byte alignment
        ptrs = tuple(P + 4 if k == i else P for k in range(6))
        assert _call(nat, ACC | 4, ptrs=ptrs) == EUNSUP, i
    # empty batch, and no coordinate set: nothing to add
    for r in range(7):
        assert _call(nat, ACC | r, B=0) == OK
        assert _call(nat, ACC | r, B=0, ptrs=(None,) * 6) == OK
    assert _call(nat, ACC | 4, Nc=0, ptrs=(P, P, None, None, P, P)) == OK
    # geometry is checked as in the unflagged call
    assert _call(nat, ACC | 4, B=-1) == EINVAL
    assert _call(nat, ACC | 4, C=0) == EINVAL
    assert lib.dxr_alt_corr_backward(P, P, P, P, P, P, 1, 0, 8, 8, 8, 64, 1, ACC | 4, None) == EINVAL
    assert lib.dxr_last_hip_error() == 0


def test_unflagged_calls_are_answered_as_before(nat):
    """The lines of tests/test_capi.py for this entry point, and the flag bit of a
    negative radius (two's complement) is not a flag."""
    EINVAL, EUNSUP, OK = nat.DXR_EINVAL, nat.DXR_EUNSUPPORTED, nat.DXR_OK
    ab = nat.load().dxr_alt_corr_backward
    assert ab(P, P, P, P, P, P, 1, 8, 8, 8, 8, 64, 1, -1, None) == EINVAL   # radius < 0
    assert ab(P, P, P, P, P, P, 1, 8, 8, 8, 8, 64, 1, 7, None) == EUNSUP    # radius > 6
    assert ab(P, P, P, P, P, P, 1, 8, 8, 8, 8, 0, 1, 4, None) == EINVAL     # C = 0
    assert ab(P, P, None, P, P, P, 1, 8, 8, 8, 8, 64, 1, 4, None) == EINVAL  # null coords
    assert ab(P, P, P, P, None, P, 1, 8, 8, 8, 8, 64, 1, 4, None) == EINVAL  # null fmap1_grad
    assert ab(None, None, None, None, None, None, 0, 8, 8, 8, 8, 64, 1, 4, None) == OK
    for r in (-1, -0x2000, -(1 << 30)):
        assert _call(nat, r) == EINVAL
        assert _call(nat, r, B=0) == EINVAL
    # every other flag of the library is still just a radius > 6 here
    for hi in (0x100, 0x200, 0x1000, 0x4000):
        assert _call(nat, hi | 4, B=0) == EUNSUP
    # C = 36 is served unflagged (B = 0: nothing launches)
    assert _call(nat, 4, B=0, C=36) == OK


def test_block_is_exported_with_the_reference_signature():
    import dexiraft_amd as dx
    from dexiraft_amd import corr

    assert "TrainableAlternateCorrBlock" in dx.__all__
    assert "TrainableAlternateCorrBlock" in corr.__all__
    T = dx.TrainableAlternateCorrBlock
    assert T is corr.TrainableAlternateCorrBlock and issubclass(T, dx.AlternateCorrBlock)
    sig = inspect.signature(T)
    assert list(sig.parameters) == ["fmap1", "fmap2", "num_levels", "radius"]
    assert sig.parameters["num_levels"].default == 4 and sig.parameters["radius"].default == 4
    assert list(inspect.signature(T.__init__).parameters) == \
        ["self", "fmap1", "fmap2", "num_levels", "radius"]
    assert list(inspect.signature(T.__call__).parameters) == ["self", "coords"]
    init = T.__init__
    assert init.__code__.co_varnames[:init.__code__.co_argcount] == \
        ("self", "fmap1", "fmap2", "num_levels", "radius")
    assert init.__defaults__ == (4, 4)
    assert init.__kwdefaults__ == {"out_dtype": None, "memory_format": None}
    # the parent's constructor is untouched
    pinit = dx.AlternateCorrBlock.__init__
    assert pinit is not init
    assert pinit.__kwdefaults__ == {"out_dtype": None, "memory_format": None}
    assert pinit.__defaults__ == (4, 4)


def test_bad_options_raise_before_the_library(monkeypatch):
    import torch

    import dexiraft_amd as dx
    from dexiraft_amd import _native as nat

    def no_launch(*a, **k):
        raise AssertionError("the native library was reached")

    monkeypatch.setattr(nat, "load", no_launch)
    f = torch.zeros(1, 16, 16, 16)
    fg = torch.zeros(1, 16, 16, 16, requires_grad=True)
    for a in (f, fg):
        for bad in (torch.float64, torch.int8, "float16", 16):
            with pytest.raises(ValueError, match="out_dtype"):
                dx.TrainableAlternateCorrBlock(a, f, out_dtype=bad)
        for bad in (torch.channels_last_3d, torch.preserve_format, "channels_last", 2):
            with pytest.raises(ValueError, match="channels_last"):
                dx.TrainableAlternateCorrBlock(a, f, memory_format=bad)
            with pytest.raises(ValueError, match="channels_last"):
                dx.TrainableAlternateCorrBlock(a, f, 4, 4, out_dtype=torch.float16,
                                               memory_format=bad)
    # host tensors are refused as everywhere, grad or not, before the library
    for a in (f, fg):
        with pytest.raises(RuntimeError, match="no CPU path"):
            dx.TrainableAlternateCorrBlock(a, f)
