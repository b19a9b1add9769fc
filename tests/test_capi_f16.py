"""CPU: the float16 input mode at the C-ABI (DXR_F16 = 2, include/dexiraft_corr.h).

Argument checks return before any launch, as in tests/test_capi.py, so these
calls are safe without a GPU.  DXR_F16 is an ``in_dtype`` of the pyramid builds
only: the set of entry points and the ABI version do not change.
"""
from __future__ import annotations

import pytest

from conftest import REPO


@pytest.fixture(scope="module")
def nat():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "_dxr_build_t16", REPO / "optical-flow_dexi-raft_amd" / "build.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build()  # no-op when fresh
    from dexiraft_amd import _native
    _native.load()
    return _native


def test_f16_code_and_abi(nat):
    assert nat.DXR_F16 == 2
    assert (nat.DXR_F32, nat.DXR_BF16) == (0, 1)
    assert nat.load().dxr_abi_version() == nat.ABI_VERSION == 10
    header = (REPO / "include" / "dexiraft_corr.h").read_text()
    assert "DXR_F16 = 2" in header
    assert "#define DXR_ABI_VERSION 10" in header


@pytest.mark.parametrize("B,D,H,W", [(1, 256, 55, 128), (8, 256, 47, 156), (2, 32, 9, 13),
                                     (1, 96, 23, 37)])
def test_f16_workspace_is_the_bf16_pack(nat, B, D, H, W):
    ws = nat.load().dxr_build_workspace_bytes
    assert ws(nat.DXR_F16, B, D, H, W) == ws(nat.DXR_BF16, B, D, H, W) > 0
    assert ws(nat.DXR_F16, B, D, H, W) >= 2 * B * D * H * W * 2


def test_f16_workspace_edge_cases(nat):
    ws = nat.load().dxr_build_workspace_bytes
    assert ws(nat.DXR_F16, 1, 48, 9, 13) == 0            # D % 32 != 0: no f16 record build
    assert ws(nat.DXR_F16, 1, 0, 9, 13) == -1            # bad geometry
    assert ws(nat.DXR_F16, 1, 32, 0, 13) == -1
    assert ws(nat.DXR_F16, -1, 32, 9, 13) == -1
    assert ws(nat.DXR_F16, 1, 32, 1 << 16, 1 << 16) == -1


def _both(nat):
    """The two build entry points with one argument list (the workspace-less one
    drops the workspace)."""
    lib = nat.load()
    P = 1 << 12  # a non-null dummy address: never dereferenced on these paths

    def plain(f1, f2, dt, lay, B, D, H, W, L, div, pyr, pdt, algo):
        return lib.dxr_corr_pyramid_build(f1, f2, dt, lay, B, D, H, W, L, div, pyr, pdt, algo, None)

    def with_ws(f1, f2, dt, lay, B, D, H, W, L, div, pyr, pdt, algo):
        return lib.dxr_corr_pyramid_build_ws(f1, f2, dt, lay, B, D, H, W, L, div, pyr, pdt, algo,
                                             P, 1 << 40, None)

    return P, (plain, with_ws)


def test_f16_statuses_match_bf16(nat):
    P, entries = _both(nat)
    EINVAL, EUNSUP = nat.DXR_EINVAL, nat.DXR_EUNSUPPORTED
    for b in entries:
        for dt in (nat.DXR_BF16, nat.DXR_F16):
            pdt = nat.DXR_BF16 if dt == nat.DXR_BF16 else nat.DXR_F32
            assert b(P, P, dt, 0, 1, 256, 7, 30, 4, 16.0, P, pdt, 0) == EINVAL     # empty level
            assert b(None, P, dt, 0, 1, 256, 8, 8, 4, 16.0, P, pdt, 0) == EINVAL   # null input
            assert b(P, None, dt, 0, 1, 256, 8, 8, 4, 16.0, P, pdt, 0) == EINVAL
            assert b(P, P, dt, 0, 1, 256, 8, 8, 4, 16.0, None, pdt, 0) == EINVAL   # null pyramid
            assert b(P, P, dt, 0, 1, 0, 8, 8, 4, 16.0, P, pdt, 0) == EINVAL        # D = 0
            assert b(P, P, dt, 2, 1, 256, 8, 8, 4, 16.0, P, pdt, 0) == EINVAL      # unknown layout
            assert b(P, P, dt, 0, 1, 256, 8, 8, 4, 16.0, P, pdt, 1) == EUNSUP      # EXACT_F32
            assert b(P, P, dt, 0, 0, 256, 8, 8, 4, 16.0, None, pdt, 0) == nat.DXR_OK   # empty batch


def test_f16_is_no_pyramid_dtype(nat):
    P, entries = _both(nat)
    for b in entries:
        for dt in (nat.DXR_F32, nat.DXR_BF16, nat.DXR_F16):
            assert b(P, P, dt, 0, 1, 256, 8, 8, 4, 16.0, P, 2, 0) == nat.DXR_EINVAL
    lib = nat.load()
    assert lib.dxr_pyramid_unpack(P, 2, 1, 8, 8, 4, 0, P, None) == nat.DXR_EINVAL
    assert lib.dxr_pyramid_pack(P, 1, 8, 8, 4, 0, P, 2, None) == nat.DXR_EINVAL
    assert lib.dxr_corr_lookup(P, 2, 1, 8, 8, 4, 4, P, P, None) == nat.DXR_EINVAL


def test_f16_requests_the_library_leaves_to_the_caller(nat):
    """Valid DXR_F16 requests outside the record build answer DXR_EUNSUPPORTED before
    any launch (CorrBlock then widens to float32): D % 32 != 0, NCHW without a
    workspace, a bf16 pyramid."""
    P, (plain, with_ws) = _both(nat)
    EUNSUP = nat.DXR_EUNSUPPORTED
    F16, BF16, F32 = nat.DXR_F16, nat.DXR_BF16, nat.DXR_F32
    for b in (plain, with_ws):
        for lay in (nat.DXR_NCHW, nat.DXR_NHWC):
            assert b(P, P, F16, lay, 1, 48, 8, 8, 4, 7.0, P, F32, 0) == EUNSUP     # D % 32 != 0
            assert b(P, P, F16, lay, 1, 256, 8, 8, 4, 16.0, P, BF16, 0) == EUNSUP  # bf16 pyramid
    assert plain(P, P, F16, nat.DXR_NCHW, 1, 256, 8, 8, 4, 16.0, P, F32, 0) == EUNSUP   # no workspace
    lib = nat.load()
    assert lib.dxr_corr_pyramid_build_ws(P, P, F16, nat.DXR_NCHW, 1, 256, 8, 8, 4, 16.0, P, F32, 0,
                                         P, 16, None) == EUNSUP                   # short workspace
    # unaligned pyramid / channels-last rows
    assert plain(P + 2, P, F16, nat.DXR_NHWC, 1, 256, 8, 8, 4, 16.0, P, F32, 0) == EUNSUP
    assert plain(P, P, F16, nat.DXR_NHWC, 1, 256, 8, 8, 4, 16.0, P + 4, F32, 0) == EUNSUP


def test_f16_elsewhere(nat):
    lib = nat.load()
    P = 1 << 12
    assert lib.dxr_corr_volume(P, P, nat.DXR_F16, 1, 256, 8, 8, 16.0, P, None) == nat.DXR_EUNSUPPORTED
    assert lib.dxr_corr_volume(P, P, nat.DXR_BF16, 1, 256, 8, 8, 16.0, P, None) == nat.DXR_EUNSUPPORTED
    # a 16-bit transpose goes as DXR_BF16; dtype 2 stays invalid there
    assert lib.dxr_transpose(P, P, 2, 1, 8, 8, None) == nat.DXR_EINVAL
