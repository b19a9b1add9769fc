"""CPU: the upsampling C-ABI (include/dexiraft_upsample.h, prefix dxu_) beside the
untouched correlation and flow ABIs, its host-side validation (every refusal
returns before any launch, so these calls are safe without a GPU), the CPU-side
refusals of ``upsample_flow``, and the float64 oracle the GPU tests compare
against (tests/upsample_oracle.py), pinned to the torch restatement of the
reference's op sequence and its autograd gradients."""
from __future__ import annotations

import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

import e2e_flow as ef
import upsample_oracle as uo
from conftest import REPO

UP_HEADER = REPO / "include" / "dexiraft_upsample.h"
FLOW_HEADER = REPO / "include" / "dexiraft_flow.h"
CORR_HEADER = REPO / "include" / "dexiraft_corr.h"
DXU = {"dxu_abi_version", "dxu_convex_upsample", "dxu_convex_upsample_backward_workspace_bytes",
       "dxu_convex_upsample_backward"}


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


def test_upsample_header_declares_exactly_four_entry_points():
    assert declared(UP_HEADER, "dxu_") == DXU
    assert declared(UP_HEADER, "dxr_") == set() and declared(UP_HEADER, "dxf_") == set()
    text = UP_HEADER.read_text()
    assert re.search(r"^#define DXU_ABI_VERSION 1$", text, re.M)
    assert "core/raft.py:87-98" in text               # the reference lines it replaces
    for name in ("DXU_MASK_F32", "DXU_MASK_F16", "DXU_MASK_BF16"):
        assert name in text


def test_library_exports_the_upsample_symbols(nat):
    out = subprocess.run(["nm", "-D", "--defined-only", str(nat.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T dxu_" in ln}
    assert exported == DXU == set(nat.UPSAMPLE_SIGNATURES)
    lib = nat.load()
    for name in DXU:
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr)
    assert lib.dxu_abi_version() == nat.UPSAMPLE_ABI_VERSION == 1


def test_correlation_and_flow_abis_are_unchanged(nat):
    out = subprocess.run(["nm", "-D", "--defined-only", str(nat.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    corr = declared(CORR_HEADER, "dxr_")
    assert len(corr) == 38 and corr == set(nat.SIGNATURES) == {s for s in syms if s.startswith("dxr_")}
    flow = declared(FLOW_HEADER, "dxf_")
    assert len(flow) == 3 and flow == set(nat.FLOW_SIGNATURES) == {s for s in syms if s.startswith("dxf_")}
    for header in (CORR_HEADER, FLOW_HEADER):
        assert declared(header, "dxu_") == set()
    assert re.search(r"^#define DXR_ABI_VERSION 10$", CORR_HEADER.read_text(), re.M)
    assert re.search(r"^#define DXF_ABI_VERSION 1$", FLOW_HEADER.read_text(), re.M)
    lib = nat.load()
    assert lib.dxr_abi_version() == nat.ABI_VERSION == 10
    assert lib.dxf_abi_version() == nat.FLOW_ABI_VERSION == 1
    tables = (set(nat.SIGNATURES), set(nat.FLOW_SIGNATURES), set(nat.UPSAMPLE_SIGNATURES))
    assert sum(map(len, tables)) == len(set().union(*tables))      # pairwise disjoint


def test_host_side_validation_needs_no_gpu(nat):
    lib = nat.load()
    fw, bw = lib.dxu_convex_upsample, lib.dxu_convex_upsample_backward
    wb = lib.dxu_convex_upsample_backward_workspace_bytes
    P = 1 << 12   # a non-null, 16-byte aligned dummy address: never dereferenced on these paths
    EINVAL, OK = nat.DXR_EINVAL, nat.DXR_OK
    F32, F16, BF16 = nat.DXU_MASK_F32, nat.DXU_MASK_F16, nat.DXU_MASK_BF16
    assert (F32, F16, BF16) == (0, 1, 2)
    BIG = 1 << 50
    # forward: (mask, mask_dtype, flow, N, H, W, out, stream)
    assert fw(None, F32, None, 0, 8, 8, None, None) == OK            # N == 0 before the pointers
    assert fw(None, 99, None, 0, -1, -1, None, None) == OK
    for geo in ((-1, 8, 8), (65536, 8, 8), (1, 0, 8), (1, 8, 0), (1, -8, -8), (1, 2048, 2049),
                (1, 1 << 22, 2), (1, 1 << 40, 1 << 40), (1, 1 << 62, 4)):
        assert fw(P, F32, P, *geo, P, None) == EINVAL, geo
        assert bw(P, P, F32, P, *geo, P, P, P, BIG, None) == EINVAL, geo
    for dt in (-1, 3, 4, 0x100):
        assert fw(P, dt, P, 1, 8, 8, P, None) == EINVAL               # unknown dtype
        assert bw(P, P, dt, P, 1, 8, 8, P, P, P, BIG, None) == EINVAL
    for dt in (F32, F16, BF16):
        assert fw(None, dt, P, 1, 8, 8, P, None) == EINVAL            # null mask
        assert fw(P, dt, None, 1, 8, 8, P, None) == EINVAL            # null flow
        assert fw(P, dt, P, 1, 8, 8, None, None) == EINVAL            # null out
    # backward: (grad_out, mask, mask_dtype, flow, N, H, W, grad_mask, grad_flow, workspace,
    #            workspace_bytes, stream)
    need = wb(2, 8, 8)
    assert need >= 72 * 2 * 8 * 8
    assert bw(None, None, F32, None, 0, 8, 8, None, None, None, 0, None) == OK
    for dt in (F32, F16, BF16):
        assert bw(None, P, dt, P, 2, 8, 8, P, P, P, need, None) == EINVAL     # null grad_out
        assert bw(P, None, dt, P, 2, 8, 8, P, P, P, need, None) == EINVAL     # null mask
        assert bw(P, P, dt, None, 2, 8, 8, P, P, P, need, None) == EINVAL     # null flow
        assert bw(P, P, dt, P, 2, 8, 8, None, None, P, need, None) == EINVAL  # no gradient asked
        assert bw(P, P, dt, P, 2, 8, 8, P, P, None, need, None) == EINVAL     # null workspace
        assert bw(P, P, dt, P, 2, 8, 8, None, P, None, need, None) == EINVAL
        assert bw(P, P, dt, P, 2, 8, 8, P, P, P + 8, need, None) == EINVAL    # not 16-byte aligned
        assert bw(P, P, dt, P, 2, 8, 8, P, P, P, need - 1, None) == EINVAL    # short
        assert bw(P, P, dt, P, 2, 8, 8, None, P, P, 0, None) == EINVAL
    assert lib.dxr_last_hip_error() == 0


def test_workspace_bytes(nat):
    """-1 for bad geometry, 0 for an empty batch, a multiple of 16, room for the
    18 T planes (72 bytes per coarse pixel), and non-decreasing in N, H and W."""
    wb = nat.load().dxu_convex_upsample_backward_workspace_bytes
    for bad in ((-1, 8, 8), (1, 0, 8), (1, 8, 0), (1, -1, -1), (65536, 8, 8), (1, 2048, 2049),
                (1, 1 << 22, 2), (1, 1 << 40, 1 << 40)):
        assert wb(*bad) == -1, bad
    assert wb(0, 8, 8) == 0
    assert wb(65535, 1, 1) > 0 and wb(1, 1 << 22, 1) > 0 and wb(65535, 2048, 2048) > 0
    for n, h, w in ((1, 1, 1), (1, 17, 19), (3, 17, 19), (1, 55, 128), (6, 46, 62), (65535, 2048, 2048)):
        b = wb(n, h, w)
        assert b % 16 == 0 and 72 * n * h * w <= b < 72 * n * h * w + 16
    dense = [wb(1, 1, n) for n in range(1, 3000)]
    assert dense == sorted(dense) and dense == [wb(1, n, 1) for n in range(1, 3000)]
    by_h = [wb(3, h, 37) for h in range(1, 400)]
    assert by_h == sorted(by_h)
    by_n = [wb(n, 55, 127) for n in (0, 1, 2, 3, 7, 8, 64, 1024, 65535)]
    assert by_n == sorted(by_n)


def test_python_wrapper_refusals():
    import dexiraft_amd as dx
    from dexiraft_amd import utils
    assert dx.upsample_flow is utils.upsample_flow
    assert "upsample_flow" in dx.__all__ and "upsample_flow" in utils.__all__
    flow, mask = torch.zeros(2, 2, 5, 7), torch.zeros(2, 576, 5, 7)
    with pytest.raises(RuntimeError, match="HIP device"):
        dx.upsample_flow(flow, mask)                                  # host tensors
    with pytest.raises(RuntimeError, match="HIP device"):
        dx.upsample_flow(flow.half(), mask.bfloat16())
    for f, m in ((flow[0], mask), (flow, mask[0]), (flow[None], mask[None]),        # ranks
                 (torch.zeros(2, 3, 5, 7), mask), (flow, torch.zeros(2, 64, 5, 7)),  # channels
                 (flow[:1], mask), (flow[:, :, :4], mask), (flow, mask[..., :6]),    # N, H, W
                 (mask, flow)):
        with pytest.raises(ValueError):
            dx.upsample_flow(f, m)
    with pytest.raises(ValueError):
        dx.upsample_flow(flow, mask.to("meta"))                       # different devices
    for dt in (torch.float64, torch.int32):
        with pytest.raises(TypeError):
            dx.upsample_flow(flow, mask.to(dt))
    with pytest.raises(TypeError):
        dx.upsample_flow(flow.double(), mask)
    with pytest.raises(TypeError):
        dx.upsample_flow(flow.numpy(), mask)


@pytest.mark.parametrize("N,H,W", [(1, 1, 1), (2, 3, 5), (1, 4, 2)])
def test_oracle_pins_itself_to_the_torch_sequence(N, H, W):
    """The numpy float64 oracle agrees to 1e-12 (relative to the largest entry of
    each tensor) with the torch restatement of core/raft.py:87-98 and its autograd
    gradients, in float64 on the CPU; -inf taps included."""
    rng = np.random.default_rng(7 + 100 * H + W)
    mask = rng.normal(0, 3, (N, 576, H, W))
    kill = rng.random((N, 9, 64, H, W)) < 0.1
    kill[:, 4] = False                                  # never a whole column
    mask[kill.reshape(N, 576, H, W)] = -np.inf
    flow = rng.normal(0, 5, (N, 2, H, W))
    gout = rng.normal(0, 1, (N, 2, 8 * H, 8 * W))
    out, scale = uo.forward(mask, flow)
    gm, gf, sm, sf = uo.backward(mask, flow, gout)
    tm = torch.from_numpy(mask).requires_grad_()
    tf = torch.from_numpy(flow).requires_grad_()
    ref = ef.upsample_flow(tf, tm)
    ref.backward(torch.from_numpy(gout))

    def close(a, b):
        b = b.detach().numpy()
        assert a.shape == b.shape and np.isfinite(a).all() and np.isfinite(b).all()
        assert np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1e-300)

    close(out, ref)
    close(gm, tm.grad)
    close(gf, tf.grad)
    assert (np.abs(out) <= scale * (1 + 1e-12)).all()
    assert (np.abs(gm) <= sm * (1 + 1e-12) + 1e-300).all() and (np.abs(gf) <= sf * (1 + 1e-12)).all()
    assert (gm.reshape(N, 9, 64, H, W)[kill] == 0).all()         # a -inf tap has weight exactly 0
