"""CPU: the sequence-loss C-ABI (include/dexiraft_loss.h, prefix dxl_) beside the
three untouched ABIs, its host-side validation (every refusal returns before any
launch, so these calls are safe without a GPU), the workspace size, the CPU-side
refusals of ``sequence_loss`` / ``flow_metrics``, and the numpy oracle the GPU
tests compare against (tests/loss_oracle.py), pinned to a float64 torch autograd
evaluation of the same definition."""
from __future__ import annotations

import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

import loss_oracle as lo
from conftest import REPO

HEADERS = {"dxl_": REPO / "include" / "dexiraft_loss.h",
           "dxu_": REPO / "include" / "dexiraft_upsample.h",
           "dxf_": REPO / "include" / "dexiraft_flow.h",
           "dxr_": REPO / "include" / "dexiraft_corr.h"}
DXL = {"dxl_abi_version", "dxl_sequence_loss_workspace_bytes", "dxl_sequence_loss",
       "dxl_sequence_loss_backward"}


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


def exported(nat) -> set[str]:
    out = subprocess.run(["nm", "-D", "--defined-only", str(nat.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if " T " in ln}


def test_loss_header_declares_exactly_four_entry_points():
    header = HEADERS["dxl_"]
    assert declared(header, "dxl_") == DXL
    for other in ("dxr_", "dxf_", "dxu_"):
        assert declared(header, other) == set()
    text = header.read_text()
    assert re.search(r"^#define DXL_ABI_VERSION 1$", text, re.M)
    assert "train.py:48-73" in text                     # the reference lines it replaces


def test_library_exports_the_loss_symbols(nat):
    syms = exported(nat)
    assert {s for s in syms if s.startswith("dxl_")} == DXL == set(nat.LOSS_SIGNATURES)
    lib = nat.load()
    for name in DXL:
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr)
    assert lib.dxl_abi_version() == nat.LOSS_ABI_VERSION == 1


def test_the_other_three_abis_are_unchanged(nat):
    syms = exported(nat)
    tables = {"dxr_": nat.SIGNATURES, "dxf_": nat.FLOW_SIGNATURES, "dxu_": nat.UPSAMPLE_SIGNATURES,
              "dxl_": nat.LOSS_SIGNATURES}
    for prefix, n in (("dxr_", 38), ("dxf_", 3), ("dxu_", 4)):
        names = declared(HEADERS[prefix], prefix)
        assert len(names) == n, prefix
        assert names == set(tables[prefix]) == {s for s in syms if s.startswith(prefix)}, prefix
        assert declared(HEADERS[prefix], "dxl_") == set()
    assert re.search(r"^#define DXR_ABI_VERSION 10$", HEADERS["dxr_"].read_text(), re.M)
    assert re.search(r"^#define DXF_ABI_VERSION 1$", HEADERS["dxf_"].read_text(), re.M)
    assert re.search(r"^#define DXU_ABI_VERSION 1$", HEADERS["dxu_"].read_text(), re.M)
    lib = nat.load()
    assert lib.dxr_abi_version() == nat.ABI_VERSION == 10
    assert lib.dxf_abi_version() == nat.FLOW_ABI_VERSION == 1
    assert lib.dxu_abi_version() == nat.UPSAMPLE_ABI_VERSION == 1
    # the four signature tables are pairwise disjoint and cover every export of the library
    assert sum(map(len, tables.values())) == len(set().union(*tables.values()))
    assert set().union(*tables.values()) == {s for s in syms if s.startswith("dx")}


def ptrs(*values):
    """A host array of pointers (None: null), as the preds / grad_preds arguments."""
    return (ctypes.c_void_p * len(values))(*values)


def test_host_side_validation_needs_no_gpu(nat):
    lib = nat.load()
    fw, bw = lib.dxl_sequence_loss, lib.dxl_sequence_loss_backward
    wb = lib.dxl_sequence_loss_workspace_bytes
    A = 1 << 12   # a non-null, 16-byte aligned dummy address: never dereferenced on these paths
    EINVAL, OK = nat.DXR_EINVAL, nat.DXR_OK
    BIG = 1 << 50
    inf, nan = float("inf"), float("nan")
    three = ptrs(A, A, A)

    # forward: (preds, P, flow_gt, valid, B, H, W, gamma, max_flow, loss, terms, stats,
    #           workspace, workspace_bytes, stream)
    def f(preds=three, P=3, gt=A, valid=A, geo=(2, 8, 8), gamma=0.8, max_flow=400.0, loss=A,
          terms=A, stats=A, ws=A, nbytes=BIG):
        return fw(preds, P, gt, valid, *geo, gamma, max_flow, loss, terms, stats, ws, nbytes, None)

    # backward: (grad_loss, preds, grad_preds, P, flow_gt, valid, B, H, W, gamma, max_flow, stream)
    def b(gl=A, preds=three, grads=three, P=3, gt=A, valid=A, geo=(2, 8, 8), gamma=0.8,
          max_flow=400.0):
        return bw(gl, preds, grads, P, gt, valid, *geo, gamma, max_flow, None)

    # B == 0 is OK before the pointers are looked at (after P and the geometry)
    assert f(preds=None, gt=None, valid=None, geo=(0, 8, 8), loss=None, terms=None, stats=None,
             ws=None, nbytes=0, gamma=nan) == OK
    assert b(gl=None, preds=None, grads=None, gt=None, valid=None, geo=(0, 8, 8), gamma=nan) == OK
    many = ptrs(*([A] * 33))
    for P in (0, -1, 33, 1 << 40):
        assert f(preds=many, P=P) == EINVAL and b(preds=many, grads=many, P=P) == EINVAL, P
        assert f(preds=many, P=P, geo=(0, 8, 8)) == EINVAL
    for geo in ((-1, 8, 8), (1, 0, 8), (1, 8, 0), (1, -8, -8), (0, 0, 8), (0, 8, -1),
                (1, 1 << 16, (1 << 15) + 1), (2, 1 << 16, 1 << 15), ((1 << 31) + 1, 1, 1),
                (1, 1 << 40, 1 << 40), (1 << 62, 4, 1), (3, 1 << 62, 1 << 62)):
        assert f(geo=geo) == EINVAL and b(geo=geo) == EINVAL, geo
    for gamma in (nan, -0.5, -inf):
        assert f(gamma=gamma) == EINVAL and b(gamma=gamma) == EINVAL
    assert f(max_flow=nan) == EINVAL and b(max_flow=nan) == EINVAL
    # null required pointers, a null entry in preds
    assert f(preds=None) == EINVAL and f(gt=None) == EINVAL
    assert b(gl=None) == EINVAL and b(preds=None) == EINVAL and b(grads=None) == EINVAL
    assert b(gt=None) == EINVAL
    for k in range(3):
        holed = ptrs(*(None if i == k else A for i in range(3)))
        assert f(preds=holed) == EINVAL and b(preds=holed) == EINVAL
    assert b(grads=ptrs(None, None, None)) == EINVAL              # no gradient asked
    assert f(loss=None, terms=None, stats=None) == EINVAL        # no output asked
    # workspace: null, misaligned, short
    need = wb(3, 2, 8, 8)
    assert need > 0
    assert f(ws=None) == EINVAL and f(ws=A + 8) == EINVAL and f(ws=A + 4) == EINVAL
    assert f(nbytes=need - 1) == EINVAL and f(nbytes=0) == EINVAL
    assert lib.dxr_last_hip_error() == 0


def test_workspace_bytes(nat):
    """-1 for the P and geometry errors, 0 for an empty batch, a multiple of 16, room
    for at least one float64 per term (and the statistics) per 2048 pixels, and
    non-decreasing in each argument."""
    wb = nat.load().dxl_sequence_loss_workspace_bytes
    for bad in ((0, 1, 8, 8), (33, 1, 8, 8), (-1, 1, 8, 8), (3, -1, 8, 8), (3, 1, 0, 8), (3, 1, 8, 0),
                (3, 1, -1, -1), (3, 2, 1 << 16, 1 << 15), (3, 1, 1 << 40, 1 << 40),
                (3, (1 << 31) + 1, 1, 1), (0, 0, 8, 8), (3, 0, 0, 8)):
        assert wb(*bad) == -1, bad
    assert wb(1, 0, 8, 8) == 0 and wb(32, 0, 1, 1) == 0
    assert wb(32, 1 << 31, 1, 1) > 0 and wb(1, 1, 1 << 16, 1 << 15) > 0 and wb(1, 1, 1, 1) > 0
    for P, B, H, W in ((1, 1, 1, 1), (3, 2, 5, 7), (12, 6, 368, 496), (32, 6, 368, 768),
                       (12, 1, 1 << 16, 1 << 15)):
        n = wb(P, B, H, W)
        assert n % 16 == 0 and n >= -(-B * H * W // 2048) * 8 * (P + 1)
    assert wb(12, 6, 368, 496) < 1 << 20           # small beside the 105 MB of predictions
    for fixed in ((2, 37, 41), (6, 368, 496)):
        by_p = [wb(P, *fixed) for P in range(1, 33)]
        assert by_p == sorted(by_p)
    dense = [wb(12, 1, 1, n) for n in range(1, 9000)]
    assert dense == sorted(dense) and dense == [wb(12, 1, n, 1) for n in range(1, 9000)]
    assert dense == [wb(12, n, 1, 1) for n in range(1, 9000)]
    by_h = [wb(3, 3, h, 37) for h in range(1, 400)]
    assert by_h == sorted(by_h)
    by_b = [wb(5, b, 55, 127) for b in (0, 1, 2, 3, 7, 8, 64, 1024, 65535)]
    assert by_b == sorted(by_b)


def test_python_wrapper_refusals():
    import dexiraft_amd as dx
    from dexiraft_amd import utils
    for name in ("sequence_loss", "flow_metrics"):
        assert getattr(dx, name) is getattr(utils, name)
        assert name in dx.__all__ and name in utils.__all__
    gt, valid = torch.zeros(2, 2, 5, 7), torch.ones(2, 5, 7)
    preds = [torch.zeros(2, 2, 5, 7) for _ in range(3)]
    with pytest.raises(RuntimeError, match="HIP device"):
        dx.sequence_loss(preds, gt, valid)                          # host tensors
    with pytest.raises(RuntimeError, match="HIP device"):
        dx.sequence_loss([p.half() for p in preds], gt, valid.bool(), sync_metrics=False)
    with pytest.raises(RuntimeError, match="HIP device"):
        dx.flow_metrics(preds[0], gt)
    with pytest.raises(RuntimeError, match="HIP device"):
        dx.flow_metrics(preds[0][0], gt[0], valid[0], 400.0)
    for p, g, v in (([], gt, valid), (preds * 11, gt, valid),                   # P = 0, 33
                    ([preds[0][0]], gt, valid), (preds, gt[0], valid),          # ranks
                    (preds, gt, valid[0]), (preds, gt, valid[:, None]),
                    (preds, torch.zeros(2, 3, 5, 7), valid),                    # channels
                    ([torch.zeros(2, 2, 5, 6)], gt, valid), (preds[:2] + [preds[0][:1]], gt, valid),
                    (preds, gt, valid[:, :4]), (preds, gt[:0], valid[:0]),      # shapes, empty
                    ([p[:0] for p in preds], gt[:0], valid[:0])):
        with pytest.raises(ValueError):
            dx.sequence_loss(p, g, v)
    with pytest.raises(ValueError):
        dx.sequence_loss(preds, gt, valid.to("meta"))               # different devices
    for bad in (dict(gamma=-1.0), dict(gamma=float("nan")), dict(max_flow=float("nan"))):
        with pytest.raises(ValueError):
            dx.sequence_loss(preds, gt, valid, **bad)
    with pytest.raises(ValueError):
        dx.flow_metrics(preds[0], gt[:, :1])
    with pytest.raises(ValueError):
        dx.flow_metrics(preds[0], gt, valid[:1])
    with pytest.raises(TypeError):
        dx.sequence_loss([p.int() for p in preds], gt, valid)
    with pytest.raises(TypeError):
        dx.sequence_loss([p.numpy() for p in preds], gt, valid)
    with pytest.raises(TypeError):
        dx.flow_metrics(preds[0], gt.numpy())


def case(B, H, W, P, seed):
    rng = np.random.default_rng(seed)
    gt = rng.normal(0, 30, (B, 2, H, W)).astype(np.float32)
    big = rng.random((B, H, W)) < 0.1
    gt[:, 0][big] = 400.0                                 # at max_flow: excluded
    gt[:, 1][big] = rng.choice([0.0, 250.0], int(big.sum()))
    valid = (rng.random((B, H, W)) < 0.8).astype(np.float32)
    preds = [(gt + rng.normal(0, 2, gt.shape)).astype(np.float32) for _ in range(P)]
    preds[-1][0, :, 0, 0] = gt[0, :, 0, 0]                # d == 0: sgn(0) = 0
    return preds, gt, valid


@pytest.mark.parametrize("B,H,W,P", [(1, 1, 1, 1), (2, 5, 7, 3), (1, 9, 4, 12)])
@pytest.mark.parametrize("gamma,max_flow", [(0.8, 400.0), (0.0, float("inf")), (1.25, 35.0)])
def test_oracle_pins_itself_to_the_torch_definition(B, H, W, P, gamma, max_flow):
    """The numpy oracle agrees to 1e-12 with a float64 torch evaluation of the
    definition and its autograd gradients (grad_loss = 2.5); the float32 gradient
    restatement is the float64 one rounded, and its counts are the float64 ones."""
    preds, gt, valid = case(B, H, W, P, 11 * H + W + P)
    loss, terms, sum_epe = lo.sums64(preds, gt, valid, gamma, max_flow)
    counts = lo.stats32(preds[-1], gt, valid, max_flow)
    tp = [torch.from_numpy(p).double().requires_grad_() for p in preds]
    tl, ts = lo.torch_sequence(tp, torch.from_numpy(gt).double(), torch.from_numpy(valid).double(),
                               gamma, max_flow)
    (2.5 * tl).backward()
    tl = tl.detach()
    assert abs(loss - float(tl)) <= 1e-12 * max(abs(float(tl)), 1e-300)
    assert abs(sum_epe - float(ts[1])) <= 1e-12 * max(float(ts[1]), 1e-300)
    assert counts[:4] == [int(ts[0]), int(ts[2]), int(ts[3]), int(ts[4])]
    w = lo.weights(P, gamma)
    assert abs(loss - sum(a * b for a, b in zip(w, terms))) <= 1e-12 * max(loss, 1e-300)
    g64 = lo.grads64(preds, gt, valid, gamma, max_flow, 2.5)
    g32 = lo.grads32(preds, gt, valid, gamma, max_flow, 2.5)
    for t, a, b in zip(tp, g64, g32):
        ref = t.grad.numpy()
        assert np.abs(a - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1e-300)
        assert b.dtype == np.float32 and np.abs(b - ref).max() <= 2.0 ** -22 * np.abs(ref).max()
        assert len(np.unique(np.abs(b))) <= 2                      # +q, -q or 0
    assert (g32[-1][0, :, 0, 0] == 0).all()
    v, mag = lo.mask32(gt, valid, max_flow)
    assert not v[mag >= max_flow].any() and not v[valid < 0.5].any()
    assert counts[0] == int(v.sum())
    # all valid when valid is None
    assert lo.mask32(gt, None, float("inf"))[0].all()
