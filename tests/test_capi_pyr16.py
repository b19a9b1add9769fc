"""CPU: the float16 pyramid dtype at the C-ABI (DXR_PYR_F16 = 4,
include/dexiraft_corr.h) and the ``pyramid_dtype`` keyword of CorrBlock.

DXR_PYR_F16 is a ``pyr_dtype`` of the pyramid builds, ``dxr_pyramid_unpack`` /
``_pack``, ``dxr_corr_lookup`` and ``dxr_corr_lookup_conv1x1`` only; the set of
entry points and the ABI version do not change.  Every call below fails an
argument check (or has an empty batch) before any launch, as in
tests/test_capi.py, so the dummy pointers are never dereferenced and the calls
are safe with or without a GPU.
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
        "_dxr_build_p16", REPO / "optical-flow_dexi-raft_amd" / "build.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build()  # no-op when fresh
    from dexiraft_amd import _native
    _native.load()
    return _native


def _build(nat, in_dt, pdt, ws=True, lay=0, B=1, D=256, H=8, W=8, L=4, f1=P, f2=P, pyr=P, algo=0,
           ws_ptr=P, ws_bytes=1 << 40):
    lib = nat.load()
    if ws:
        return lib.dxr_corr_pyramid_build_ws(f1, f2, in_dt, lay, B, D, H, W, L, 16.0, pyr, pdt, algo,
                                             ws_ptr, ws_bytes, None)
    return lib.dxr_corr_pyramid_build(f1, f2, in_dt, lay, B, D, H, W, L, 16.0, pyr, pdt, algo, None)


def _unpack(nat, dt, B=1, H=8, W=8, L=4, lvl=0, pyr=P, out=P):
    return nat.load().dxr_pyramid_unpack(pyr, dt, B, H, W, L, lvl, out, None)


def _pack(nat, dt, B=1, H=8, W=8, L=4, lvl=0, pyr=P, src=P):
    return nat.load().dxr_pyramid_pack(src, B, H, W, L, lvl, pyr, dt, None)


def _lookup(nat, dt, B=1, H=8, W=8, L=4, r=4, pyr=P, coords=P, out=P):
    return nat.load().dxr_corr_lookup(pyr, dt, B, H, W, L, r, coords, out, None)


def _conv(nat, dt, B=1, H=8, W=8, L=4, r=4, pyr=P, coords=P, wpk=P, out=P, cout=96):
    return nat.load().dxr_corr_lookup_conv1x1(pyr, dt, B, H, W, L, r, coords, wpk, None, cout, 1,
                                              out, None)


def test_code_header_abi_and_entry_points(nat):
    assert nat.DXR_PYR_F16 == 4
    header = (REPO / "include" / "dexiraft_corr.h").read_text()
    assert "DXR_PYR_F16 = 4" in header
    assert "DXR_F16 = 2" in header
    assert "#define DXR_ABI_VERSION 10" in header
    assert nat.load().dxr_abi_version() == nat.ABI_VERSION == 10
    assert set(nat.SIGNATURES) == set(DECL.findall(header))


@pytest.mark.parametrize("ws", [False, True])
def test_build_statuses_match_the_bf16_pyramid(nat, ws):
    """in_dtype F16 and F32 (+ workspace) into DXR_PYR_F16 against the bf16 fmaps
    -> bf16 pyramid call: the shared argument checks answer alike."""
    EINVAL, OK = nat.DXR_EINVAL, nat.DXR_OK
    BF, PF = nat.DXR_BF16, nat.DXR_PYR_F16
    for in_dt in (nat.DXR_F16, nat.DXR_F32):
        for kw in (dict(H=7, W=30),              # empty level
                   dict(f1=None), dict(f2=None), dict(pyr=None),
                   dict(D=0), dict(lay=2), dict(algo=2)):
            assert _build(nat, BF, BF, ws, **kw) == EINVAL == _build(nat, in_dt, PF, ws, **kw), kw
        assert _build(nat, BF, BF, ws, B=0, pyr=None) == OK == _build(nat, in_dt, PF, ws, B=0,
                                                                     pyr=None)


def test_unpack_pack_statuses_match_the_bf16_pyramid(nat):
    EINVAL, OK = nat.DXR_EINVAL, nat.DXR_OK
    BF, PF = nat.DXR_BF16, nat.DXR_PYR_F16
    for call, other in ((_unpack, "out"), (_pack, "src")):
        for kw in (dict(H=7, W=30), dict(pyr=None), {other: None}, dict(lvl=4), dict(lvl=-1)):
            assert call(nat, BF, **kw) == EINVAL == call(nat, PF, **kw), (call.__name__, kw)
        assert call(nat, BF, B=0, pyr=None) == OK == call(nat, PF, B=0, pyr=None)


@pytest.mark.parametrize("entry", ["lookup", "conv1x1"])
def test_lookup_statuses_match_the_bf16_pyramid(nat, entry):
    call = _lookup if entry == "lookup" else _conv
    EINVAL, EUNSUP, OK = nat.DXR_EINVAL, nat.DXR_EUNSUPPORTED, nat.DXR_OK
    for flag in (0, nat.DXR_OUT_F16, nat.DXR_OUT_BF16):
        bf, pf = flag | nat.DXR_BF16, flag | nat.DXR_PYR_F16
        assert call(nat, bf, H=7, W=30) == EINVAL == call(nat, pf, H=7, W=30)   # empty level
        assert call(nat, bf, pyr=None) == EINVAL == call(nat, pf, pyr=None)
        assert call(nat, bf, coords=None) == EINVAL == call(nat, pf, coords=None)
        assert call(nat, bf, out=None) == EINVAL == call(nat, pf, out=None)
        assert call(nat, bf, r=-1) == EINVAL == call(nat, pf, r=-1)
        assert call(nat, bf, r=9) == EUNSUP == call(nat, pf, r=9)
        assert call(nat, bf, B=0) == OK == call(nat, pf, B=0)
        assert call(nat, bf, B=0, out=None) == OK == call(nat, pf, B=0, out=None)
        if flag:   # 16-bit outputs: an odd address is refused on the host
            assert call(nat, pf, out=P + 1) == EINVAL
    # the bad flag combinations stay bad on the new low value
    assert call(nat, 0x300 | nat.DXR_PYR_F16) == EINVAL
    assert call(nat, 0x400 | nat.DXR_PYR_F16) == EINVAL
    assert call(nat, 0x10000 | nat.DXR_PYR_F16) == EINVAL
    if entry == "conv1x1":
        assert _conv(nat, nat.DXR_PYR_F16, wpk=None) == EINVAL
        assert _conv(nat, nat.DXR_PYR_F16, cout=48) == EUNSUP
        assert _conv(nat, nat.DXR_PYR_F16, r=2) == EUNSUP


def test_requests_left_to_the_caller_are_unsupported_before_launch(nat):
    EUNSUP = nat.DXR_EUNSUPPORTED
    F32, BF, F16, PF = nat.DXR_F32, nat.DXR_BF16, nat.DXR_F16, nat.DXR_PYR_F16
    for ws in (False, True):
        for lay in (nat.DXR_NCHW, nat.DXR_NHWC):
            assert _build(nat, BF, PF, ws, lay=lay) == EUNSUP                 # bf16 fmaps
            assert _build(nat, BF, PF, ws, lay=lay, D=48) == EUNSUP
            assert _build(nat, F32, PF, ws, lay=lay, algo=1) == EUNSUP        # EXACT_F32
            assert _build(nat, F16, PF, ws, lay=lay, algo=1) == EUNSUP
            assert _build(nat, F32, PF, ws, lay=lay, H=32, W=32, L=5) == EUNSUP   # 5 levels
            assert _build(nat, F16, PF, ws, lay=lay, H=32, W=32, L=5) == EUNSUP
            assert _build(nat, F16, PF, ws, lay=lay, D=48) == EUNSUP          # D % 32 != 0
            assert _build(nat, F32, PF, ws, lay=lay, D=40) == EUNSUP          # D % 16 != 0
        assert _build(nat, F32, PF, False, lay=nat.DXR_NCHW) == EUNSUP        # f32, no workspace
        assert _build(nat, F32, PF, False, lay=nat.DXR_NHWC) == EUNSUP
    assert _build(nat, F32, PF, True, ws_ptr=None, ws_bytes=0) == EUNSUP
    assert _build(nat, F32, PF, True, ws_bytes=16) == EUNSUP                  # short workspace
    assert _build(nat, F16, PF, False, lay=nat.DXR_NCHW) == EUNSUP            # NCHW f16 needs one
    assert _build(nat, F16, PF, True, ws_bytes=16) == EUNSUP
    assert _build(nat, F32, PF, True, pyr=P + 4) == EUNSUP                    # unaligned pyramid
    assert _build(nat, F16, PF, True, lay=nat.DXR_NHWC, pyr=P + 4) == EUNSUP
    assert _build(nat, F16, PF, True, lay=nat.DXR_NHWC, f1=P + 2) == EUNSUP   # unaligned rows


def test_pyr_f16_is_no_in_dtype_and_no_dtype_elsewhere(nat):
    lib = nat.load()
    EINVAL = nat.DXR_EINVAL
    PF = nat.DXR_PYR_F16
    for ws in (False, True):
        for pdt in (nat.DXR_F32, nat.DXR_BF16, PF):
            assert _build(nat, PF, pdt, ws) == EINVAL
    assert lib.dxr_build_workspace_bytes(PF, 1, 256, 8, 8) == 0
    assert lib.dxr_corr_volume(P, P, PF, 1, 256, 8, 8, 16.0, P, None) == EINVAL
    assert lib.dxr_corr_lookup_backward(P, P, 1, 8, 8, 4, 4, P, PF, None) == EINVAL
    cs = (nat._vp * 1)(P)
    assert lib.dxr_corr_lookup_backward_multi(cs, cs, 1, 1, 8, 8, 4, 4, P, PF, None) == EINVAL
    assert lib.dxr_corr_lookup_backward_multi_bound(cs, cs, 1, 1, 8, 8, 4, 4, P, PF, P,
                                                    None) == EINVAL
    assert lib.dxr_pyramid_backward(P, PF, 1, 8, 8, 4, 16.0, P, None) == EINVAL
    assert lib.dxr_fmap_grads(P, PF, P, P, 1, 256, 8, 8, 4, 16.0, P, P, P, 1 << 40, None) == EINVAL
    assert lib.dxr_fmap_grads_bounded(P, PF, P, P, 1, 256, 8, 8, 4, 16.0, P, 1, P, P, P, 1 << 40,
                                      None) == EINVAL
    assert lib.dxr_transpose(P, P, PF, 1, 8, 8, None) == EINVAL
    # the neighbouring codes keep their answers
    for dt in (2, 3, 5, 7):
        assert _unpack(nat, dt) == EINVAL and _pack(nat, dt) == EINVAL
        assert _lookup(nat, dt) == EINVAL and _conv(nat, dt) == EINVAL
        assert _build(nat, nat.DXR_F32, dt) == EINVAL


def test_python_interface_declares_pyramid_dtype():
    """``pyramid_dtype`` is the fifth constructor argument (default None); the
    reported signature stays the reference's four (tests/test_api_cpu.py);
    AlternateCorrBlock has no such argument.  Validation without a GPU through the
    helper the constructor calls."""
    import inspect

    import torch

    import dexiraft_amd as dx
    from dexiraft_amd.corr import _f16_pyramid
    code = dx.CorrBlock.__init__.__code__
    assert code.co_varnames[:code.co_argcount] == ("self", "fmap1", "fmap2", "num_levels", "radius",
                                                   "pyramid_dtype")
    assert dx.CorrBlock.__init__.__defaults__ == (4, 4, None)
    sig = inspect.signature(dx.CorrBlock.__init__)
    assert list(sig.parameters) == ["self", "fmap1", "fmap2", "num_levels", "radius"]
    assert sig.parameters["num_levels"].default == 4 and sig.parameters["radius"].default == 4
    alt = dx.AlternateCorrBlock.__init__.__code__
    assert alt.co_varnames[:alt.co_argcount] == ("self", "fmap1", "fmap2", "num_levels", "radius")
    assert "pyramid_dtype" in dx.CorrBlock.__doc__

    for fm in (torch.float32, torch.float16, torch.bfloat16):
        assert _f16_pyramid(fm, None) is False
    for fm in (torch.float32, torch.float16):
        assert _f16_pyramid(fm, torch.float32) is False
        assert _f16_pyramid(fm, torch.float16) is True
    for bad in (torch.bfloat16, torch.float64, torch.int16, "float16", 16, True):
        with pytest.raises(ValueError, match="pyramid_dtype"):
            _f16_pyramid(torch.float16, bad)
    for dt in (torch.float16, torch.float32):     # contradicts the fmap dtype
        with pytest.raises(ValueError, match="bfloat16"):
            _f16_pyramid(torch.bfloat16, dt)
