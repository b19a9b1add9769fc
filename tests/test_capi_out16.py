"""CPU: the output dtype flags of the lookup at the C-ABI (DXR_OUT_F16 = 0x100,
DXR_OUT_BF16 = 0x200, include/dexiraft_corr.h).

They are or-ed onto the ``pyr_dtype`` of ``dxr_corr_lookup`` and
``dxr_corr_lookup_conv1x1`` only; the set of entry points and the ABI version do
not change.  Argument checks return before any launch, as in tests/test_capi.py,
so these calls are safe without a GPU.
"""
from __future__ import annotations

import re

import pytest

from conftest import REPO

DECL = re.compile(r"^\s*(?:int|int64_t|const char\*)\s+(dxr_\w+)\s*\(", re.M)
P = 1 << 12   # a non-null, aligned dummy address: never dereferenced on these paths


@pytest.fixture(scope="module")
def nat():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "_dxr_build_o16", REPO / "optical-flow_dexi-raft_amd" / "build.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build()  # no-op when fresh
    from dexiraft_amd import _native
    _native.load()
    return _native


def _lookup(nat, dt, B=1, H=8, W=8, L=4, r=4, pyr=P, coords=P, out=P):
    return nat.load().dxr_corr_lookup(pyr, dt, B, H, W, L, r, coords, out, None)


def _conv(nat, dt, B=1, H=8, W=8, L=4, r=4, pyr=P, coords=P, wpk=P, out=P, cout=96):
    return nat.load().dxr_corr_lookup_conv1x1(pyr, dt, B, H, W, L, r, coords, wpk, None, cout, 1,
                                              out, None)


def test_flag_values_and_header(nat):
    assert nat.DXR_OUT_F16 == 0x100
    assert nat.DXR_OUT_BF16 == 0x200
    header = (REPO / "include" / "dexiraft_corr.h").read_text()
    assert "#define DXR_OUT_F16 0x100" in header
    assert "#define DXR_OUT_BF16 0x200" in header


def test_abi_and_entry_points_unchanged(nat):
    assert nat.load().dxr_abi_version() == nat.ABI_VERSION == 10
    header = (REPO / "include" / "dexiraft_corr.h").read_text()
    assert "#define DXR_ABI_VERSION 10" in header
    assert set(nat.SIGNATURES) == set(DECL.findall(header))
    assert hasattr(nat, "DXR_OUT_F16") and hasattr(nat, "DXR_OUT_BF16")


@pytest.mark.parametrize("entry", ["lookup", "conv1x1"])
def test_bad_flag_combinations_are_einval(nat, entry):
    call = _lookup if entry == "lookup" else _conv
    EINVAL = nat.DXR_EINVAL
    assert call(nat, 0x300) == EINVAL                               # both flags, on DXR_F32
    assert call(nat, 0x300 | nat.DXR_BF16) == EINVAL
    assert call(nat, 0x400 | nat.DXR_F32) == EINVAL                 # another high bit
    assert call(nat, 0x400 | nat.DXR_OUT_F16 | nat.DXR_F32) == EINVAL
    assert call(nat, 0x10000 | nat.DXR_BF16) == EINVAL
    assert call(nat, nat.DXR_OUT_F16 | 2) == EINVAL                 # DXR_F16 is no pyr_dtype
    assert call(nat, nat.DXR_OUT_BF16 | 2) == EINVAL
    assert call(nat, nat.DXR_OUT_F16 | 3) == EINVAL
    assert call(nat, 2) == EINVAL                                   # as before the flags


def test_flags_are_invalid_at_other_entry_points(nat):
    lib = nat.load()
    EINVAL = nat.DXR_EINVAL
    for flag in (nat.DXR_OUT_F16, nat.DXR_OUT_BF16):
        for low in (nat.DXR_F32, nat.DXR_BF16):
            dt = flag | low
            assert lib.dxr_pyramid_unpack(P, dt, 1, 8, 8, 4, 0, P, None) == EINVAL
            assert lib.dxr_pyramid_pack(P, 1, 8, 8, 4, 0, P, dt, None) == EINVAL
            assert lib.dxr_corr_pyramid_build(P, P, nat.DXR_F32, 0, 1, 256, 8, 8, 4, 16.0, P, dt, 0,
                                              None) == EINVAL
            assert lib.dxr_corr_pyramid_build(P, P, dt, 0, 1, 256, 8, 8, 4, 16.0, P, nat.DXR_F32, 0,
                                              None) == EINVAL
            assert lib.dxr_corr_lookup_backward(P, P, 1, 8, 8, 4, 4, P, dt, None) == EINVAL
            assert lib.dxr_pyramid_backward(P, dt, 1, 8, 8, 4, 16.0, P, None) == EINVAL
            assert lib.dxr_transpose(P, P, dt, 1, 8, 8, None) == EINVAL


@pytest.mark.parametrize("entry", ["lookup", "conv1x1"])
def test_flagged_calls_keep_the_unflagged_checks(nat, entry):
    call = _lookup if entry == "lookup" else _conv
    EINVAL = nat.DXR_EINVAL
    for flag in (nat.DXR_OUT_F16, nat.DXR_OUT_BF16):
        for low in (nat.DXR_F32, nat.DXR_BF16):
            dt = flag | low
            # the unflagged call's answers, one for one
            assert call(nat, low, H=7, W=30) == EINVAL == call(nat, dt, H=7, W=30)   # empty level
            assert call(nat, low, out=None) == EINVAL == call(nat, dt, out=None)     # null out
            assert call(nat, low, pyr=None) == EINVAL == call(nat, dt, pyr=None)
            assert call(nat, low, coords=None) == EINVAL == call(nat, dt, coords=None)
            assert call(nat, low, r=-1) == EINVAL == call(nat, dt, r=-1)
            assert call(nat, low, r=9) == nat.DXR_EUNSUPPORTED == call(nat, dt, r=9)
            # empty batch: nothing to do, as the unflagged call
            assert call(nat, low, B=0) == nat.DXR_OK == call(nat, dt, B=0)
            assert call(nat, dt, B=0, out=None) == call(nat, low, B=0, out=None) == nat.DXR_OK
            # 16-bit elements need 2-byte alignment, nothing stronger (checked on the
            # host: an odd address is refused; P + 2 passes every check up to the
            # null-pointer test that follows it)
            assert call(nat, dt, out=P + 1) == EINVAL
            assert call(nat, dt, out=P + 2, pyr=None) == EINVAL
    if entry == "conv1x1":
        assert _conv(nat, nat.DXR_OUT_F16 | nat.DXR_F32, wpk=None) == EINVAL
        assert _conv(nat, nat.DXR_OUT_F16 | nat.DXR_F32, cout=48) == nat.DXR_EUNSUPPORTED


def test_python_interface_declares_out_dtype():
    """CPU side of the Python interface: the keyword exists where the feature is
    (CorrBlock.__call__ and lookup_conv1x1, default None) and nowhere else.  The
    reported signature of __call__ stays the reference's (tests/test_api_cpu.py)."""
    import inspect

    import dexiraft_amd as dx
    code = dx.CorrBlock.__call__.__code__
    assert code.co_varnames[:code.co_argcount] == ("self", "coords", "out_dtype")
    assert dx.CorrBlock.__call__.__defaults__ == (None,)
    sig = inspect.signature(dx.CorrBlock.lookup_conv1x1)
    assert list(sig.parameters) == ["self", "coords", "weight", "bias", "relu", "out_dtype"]
    assert sig.parameters["out_dtype"].default is None
    alt = dx.AlternateCorrBlock.__call__.__code__
    assert alt.co_varnames[:alt.co_argcount] == ("self", "coords")
    from dexiraft_amd.corr import _out_flag
    import torch
    assert _out_flag(None) == (torch.float32, 0) == _out_flag(torch.float32)
    assert _out_flag(torch.float16) == (torch.float16, 0x100)
    assert _out_flag(torch.bfloat16) == (torch.bfloat16, 0x200)
    for bad in (torch.float64, torch.int16, "float16", 16):
        with pytest.raises(ValueError, match="float16"):
            _out_flag(bad)
