"""CPU: the flow C-ABI (include/dexiraft_flow.h, prefix dxf_) beside the untouched
correlation ABI, its host-side validation (every refusal returns before any
launch, so these calls are safe without a GPU), and the CPU-side refusals of
``forward_interpolate`` and ``driver.infer_sequence``."""
from __future__ import annotations

import ctypes
import re
import subprocess

import pytest
import torch

from conftest import REPO

FLOW_HEADER = REPO / "include" / "dexiraft_flow.h"
CORR_HEADER = REPO / "include" / "dexiraft_corr.h"
DXF = {"dxf_abi_version", "dxf_forward_interpolate_workspace_bytes", "dxf_forward_interpolate"}


def declared(header, prefix: str) -> set[str]:
    pat = re.compile(r"^\s*(?:int|int64_t|const char\*)\s+(" + prefix + r"\w+)\s*\(", re.M)
    return set(pat.findall(header.read_text()))


@pytest.fixture(scope="module")
def nat():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "_dxr_build_t", REPO / "optical-flow_dexi-raft_amd" / "build.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build()  # no-op when fresh
    from dexiraft_amd import _native
    _native.load()
    return _native


def test_flow_header_declares_exactly_three_entry_points():
    assert declared(FLOW_HEADER, "dxf_") == DXF
    assert declared(FLOW_HEADER, "dxr_") == set()
    text = FLOW_HEADER.read_text()
    assert re.search(r"^#define DXF_ABI_VERSION 1$", text, re.M)
    assert "core/utils/utils.py:26-54" in text        # the reference lines it replaces


def test_library_exports_the_flow_symbols(nat):
    out = subprocess.run(["nm", "-D", "--defined-only", str(nat.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T dxf_" in ln}
    assert exported == DXF == set(nat.FLOW_SIGNATURES)
    lib = nat.load()
    for name in DXF:
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr)
    assert lib.dxf_abi_version() == nat.FLOW_ABI_VERSION == 1


def test_correlation_abi_is_unchanged(nat):
    corr = declared(CORR_HEADER, "dxr_")
    assert len(corr) == 38 and corr == set(nat.SIGNATURES)
    assert declared(CORR_HEADER, "dxf_") == set()
    assert re.search(r"^#define DXR_ABI_VERSION 10$", CORR_HEADER.read_text(), re.M)
    assert nat.load().dxr_abi_version() == nat.ABI_VERSION == 10
    assert not (set(nat.SIGNATURES) & set(nat.FLOW_SIGNATURES))


def test_host_side_validation_needs_no_gpu(nat):
    lib = nat.load()
    fi, wb = lib.dxf_forward_interpolate, lib.dxf_forward_interpolate_workspace_bytes
    P = 1 << 12   # a non-null, 16-byte aligned dummy address: never dereferenced on these paths
    EINVAL, OK = nat.DXR_EINVAL, nat.DXR_OK
    need = wb(1, 8, 8)
    assert need > 0
    # (flow, B, H, W, out, workspace, workspace_bytes, stream)
    assert fi(None, 0, 8, 8, None, None, 0, None) == OK              # B == 0 before the pointers
    assert fi(None, 1, 8, 8, P, P, need, None) == EINVAL             # null flow
    assert fi(P, 1, 8, 8, None, P, need, None) == EINVAL             # null out
    assert fi(P, 1, 0, 8, P, P, need, None) == EINVAL                # H < 1
    assert fi(P, 1, 8, 0, P, P, need, None) == EINVAL                # W < 1
    assert fi(P, 1, -8, -8, P, P, need, None) == EINVAL
    assert fi(P, -1, 8, 8, P, P, need, None) == EINVAL               # B < 0
    big = wb(1, 2048, 2048)
    assert big > 0
    assert fi(P, 1, 2048, 2049, P, P, 1 << 40, None) == EINVAL       # H*W > 2^22
    assert fi(P, 1, 1 << 40, 1 << 40, P, P, 1 << 40, None) == EINVAL  # H*W overflows
    assert fi(P, 65536, 8, 8, P, P, 1 << 40, None) == EINVAL         # B > 65535
    assert fi(P, 1, 8, 8, P, None, need, None) == EINVAL             # null workspace
    assert fi(P, 1, 8, 8, P, P + 8, need, None) == EINVAL            # not 16-byte aligned
    assert fi(P, 1, 8, 8, P, P, need - 1, None) == EINVAL            # short
    assert fi(P, 3, 8, 8, P, P, wb(3, 8, 8) - 1, None) == EINVAL
    assert lib.dxr_last_hip_error() == 0


def test_workspace_bytes(nat):
    """-1 for bad geometry, 0 for an empty batch, a multiple of 16, room for the
    landing positions (16 B per source) and at least one (d2, index) partial per
    grid point, and non-decreasing in B, H and W."""
    wb = nat.load().dxf_forward_interpolate_workspace_bytes
    for bad in ((-1, 8, 8), (1, 0, 8), (1, 8, 0), (1, -1, -1), (65536, 8, 8), (1, 2048, 2049),
                (1, 1 << 22, 2), (1, 1 << 40, 1 << 40)):
        assert wb(*bad) == -1, bad
    assert wb(0, 8, 8) == 0
    assert wb(65535, 1, 1) > 0 and wb(1, 1 << 22, 1) > 0 and wb(1, 2048, 2048) > 0
    for b, h, w in ((1, 1, 1), (1, 17, 19), (3, 17, 19), (1, 55, 128), (2, 135, 240)):
        n = wb(b, h, w)
        assert n % 16 == 0 and n >= b * h * w * (16 + 12)
        assert n == b * wb(1, h, w)
    sizes = [1, 2, 3, 15, 16, 17, 255, 256, 257, 511, 512, 513, 1000, 7040, 8191, 8192, 8193,
             32400, 65536, 262143, 262144, 262145, 1 << 20, (1 << 22) - 1, 1 << 22]
    by_w = [wb(1, 1, n) for n in sizes]
    assert by_w == sorted(by_w) and by_w == [wb(1, n, 1) for n in sizes]
    dense = [wb(1, 1, n) for n in range(1, 3000)]
    assert dense == sorted(dense)
    by_h = [wb(2, h, 37) for h in range(1, 400)]
    assert by_h == sorted(by_h)
    by_b = [wb(b, 55, 128) for b in (0, 1, 2, 3, 7, 8, 64, 1024, 65535)]
    assert by_b == sorted(by_b)


def test_python_wrapper_refusals():
    import dexiraft_amd as dx
    from dexiraft_amd import utils
    assert dx.forward_interpolate is utils.forward_interpolate
    assert "forward_interpolate" in dx.__all__ and "forward_interpolate" in utils.__all__
    with pytest.raises(RuntimeError, match="HIP device"):
        dx.forward_interpolate(torch.zeros(2, 5, 7))                  # host tensor
    with pytest.raises(RuntimeError, match="HIP device"):
        dx.forward_interpolate(torch.zeros(3, 2, 5, 7))
    for shape in ((5, 7), (3, 5, 7), (1, 3, 5, 7), (2, 2, 2, 5, 7), (2,)):
        with pytest.raises(ValueError):
            dx.forward_interpolate(torch.zeros(shape))                # rank / channel count
    with pytest.raises(NotImplementedError):
        dx.forward_interpolate(torch.zeros(2, 5, 7, requires_grad=True))
    with torch.no_grad(), pytest.raises(RuntimeError, match="HIP device"):
        dx.forward_interpolate(torch.zeros(2, 5, 7, requires_grad=True))   # past the grad check


def test_infer_sequence_refuses_short_sequences():
    from dexiraft_amd import driver
    assert "infer_sequence" in driver.__all__

    def model(*a, **k):
        raise AssertionError("the model must not be called")
    for frames in (torch.zeros(1, 3, 16, 16), torch.zeros(0, 3, 16, 16)):
        with pytest.raises(ValueError):
            driver.infer_sequence(model, frames)
    with pytest.raises(ValueError):
        driver.infer_sequence(model, torch.zeros(3, 16, 16))          # not [T, 3, H, W]
