"""GPU: ``dexiraft_amd.upsample_flow`` (csrc/flow_upsample.hip, reference
core/raft.py:87-98), forward and backward.

Shapes (N, H, W): a single pixel (all 8 outer taps padded), one row, one column,
and two maps past one and past two 64-lane tiles that are multiples of neither.
The kernels' lanes run along the flat pixel index h*W + w, 64 pixels per
workgroup, so (2, 5, 67) is 335 pixels = 5 full tiles + 15 with rows that start
inside a wave, and (1, 9, 130) is 1170 pixels = 18 tiles + 18; the widths past 64
and 128 are kept as the issue lists them.

Exact tests (``torch.equal``): one-hot masks (tap order, (i, j) placement, the
padding), 16-bit masks against the float32 call on ``mask.float()``,
determinism, the scalar path taken for pointers that are not 16-byte aligned,
and graph replay against eager.

Tolerances against the numpy float64 oracle (tests/upsample_oracle.py, pinned on
the CPU by tests/test_upsample_cpu.py) are derived, not measured.  With
u = 2^-24: forward |out - ref| <= 1e-5 * sum_k w_k |8 f_{c,k}| + 1e-37 (the
rounding budget is about 25u ~ 1.5e-6 of that sum: subtraction, exp to a few
ulp, a 9-term sum, the division and a 9-term dot product); grad_mask
<= 1e-5 * w_k (A_k + sum_m w_m A_m) + 1e-37 with A_k = sum_c |g_c| |8 f_{c,k}|;
grad_flow <= 1e-4 * 8 sum w_k |g_c| + 1e-37 over its 576-term index set (worst
sequential sum (576 - 1 + 25)u ~ 3.6e-5).  Each test prints the largest fraction
of its bound that was used.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest
import torch

import upsample_oracle as uo

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(1, 1, 1), (1, 1, 5), (2, 3, 1), (2, 5, 67), (1, 9, 130)]
KINDS = ["normal", "wide", "neg_inf", "equal"]
TOL_OUT, TOL_MASK, TOL_FLOW, TOL_ABS = 1e-5, 1e-5, 1e-4, 1e-37


@pytest.fixture(scope="module")
def dx():
    import dexiraft_amd
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    dexiraft_amd.load_native()
    return dexiraft_amd


@lru_cache(maxsize=None)
def inputs(shape, kind="normal"):
    """(mask, flow, grad_out) float32 numpy: masks N(0, 1) / N(0, 30^2) / N(0, 1) with
    about 10 % of the taps at -inf but never a whole column / all equal; flows
    N(0, 5^2); grad_out N(0, 1).  Cached and never modified."""
    N, H, W = shape
    rng = np.random.default_rng(1000 * KINDS.index(kind) + 100 * H + W + N)
    if kind == "equal":
        mask = np.full((N, 576, H, W), 0.75, dtype=np.float32)
    else:
        mask = rng.normal(0, 30.0 if kind == "wide" else 1.0, (N, 576, H, W)).astype(np.float32)
    if kind == "neg_inf":
        kill = rng.random((N, 9, 64, H, W)) < 0.1
        kill[:, rng.integers(0, 9)] = False
        mask[kill.reshape(N, 576, H, W)] = -np.inf
    flow = rng.normal(0, 5.0, (N, 2, H, W)).astype(np.float32)
    gout = rng.normal(0, 1.0, (N, 2, 8 * H, 8 * W)).astype(np.float32)
    for a in (mask, flow, gout):
        a.setflags(write=False)
    return mask, flow, gout


@lru_cache(maxsize=None)
def oracle(shape, kind):
    mask, flow, gout = inputs(shape, kind)
    return uo.forward(mask, flow) + uo.backward(mask, flow, gout)


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def run(dx, mask, flow, gout, want=("flow", "mask")):
    """(out, grad_flow, grad_mask) through the public function; None where not asked."""
    f = flow.clone().requires_grad_("flow" in want)
    m = mask.clone().requires_grad_("mask" in want)
    out = dx.upsample_flow(f, m)
    out.backward(gout)
    torch.cuda.synchronize()
    return out.detach(), f.grad, m.grad


def shifted(flow, k):
    """8 * flow moved by tap k with zeros where the tap leaves the map: [N, 2, H, W]."""
    N, _, H, W = flow.shape
    pad = torch.nn.functional.pad(8 * flow, (1, 1, 1, 1))
    return pad[:, :, k // 3:k // 3 + H, k % 3:k % 3 + W]


@pytest.mark.parametrize("shape", SHAPES)
def test_one_hot_mask_selects_the_shifted_flow(dx, shape):
    N, H, W = shape
    flow = dev(inputs(shape)[1])
    for k in range(9):
        mask = torch.zeros(N, 9, 64, H, W, device=DEV)
        mask[:, k] = 200.0
        with torch.no_grad():
            out = dx.upsample_flow(flow, mask.view(N, 576, H, W))
        want = shifted(flow, k).repeat_interleave(8, dim=2).repeat_interleave(8, dim=3)
        assert torch.equal(out, want), k


@pytest.mark.parametrize("shape", SHAPES)
def test_one_hot_per_subpixel_pins_the_channel_index(dx, shape):
    """Channel 64k + 8i + j: the hot tap of sub-pixel (i, j) is (8i + j) % 9."""
    N, H, W = shape
    flow = dev(inputs(shape)[1])
    mask = torch.zeros(N, 576, H, W, device=DEV)
    want = torch.empty(N, 2, 8 * H, 8 * W, device=DEV)
    for i in range(8):
        for j in range(8):
            k = (8 * i + j) % 9
            mask[:, 64 * k + 8 * i + j] = 200.0
            want[:, :, i::8, j::8] = shifted(flow, k)
    with torch.no_grad():
        out = dx.upsample_flow(flow, mask)
    assert torch.equal(out, want)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("shape", SHAPES)
def test_16_bit_masks_are_the_float32_computation_on_the_widened_mask(dx, shape, dtype):
    mask, flow, gout = (dev(a) for a in inputs(shape))
    m16 = mask.to(dtype)
    out16, gf16, gm16 = run(dx, m16, flow, gout)
    out32, gf32, gm32 = run(dx, m16.float(), flow, gout)
    assert gm16.dtype == dtype and out16.dtype == gf16.dtype == torch.float32
    assert torch.equal(out16, out32)
    assert torch.equal(gf16, gf32)
    assert torch.equal(gm16, gm32.to(dtype))


@pytest.mark.parametrize("shape", SHAPES)
def test_deterministic_and_grad_flow_independent_of_grad_mask(dx, shape):
    mask, flow, gout = (dev(a) for a in inputs(shape, "wide"))
    a = run(dx, mask, flow, gout)
    b = run(dx, mask, flow, gout)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    _, gf, gm = run(dx, mask, flow, gout, want=("flow",))
    assert gm is None and torch.equal(gf, a[1])
    _, gf, gm = run(dx, mask, flow, gout, want=("mask",))
    assert gf is None and torch.equal(gm, a[2])


def used(got, ref, scale, tol):
    """Largest |got - ref| / (tol * scale + TOL_ABS); the test passes when it is <= 1."""
    got = got.double().cpu().numpy()
    assert got.shape == ref.shape and np.isfinite(got).all()
    return float((np.abs(got - ref) / (tol * scale + TOL_ABS)).max())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_against_the_float64_oracle(dx, shape, kind):
    mask, flow, gout = (dev(a) for a in inputs(shape, kind))
    ref_out, s_out, ref_gm, ref_gf, s_gm, s_gf = oracle(shape, kind)
    out, gf, gm = run(dx, mask, flow, gout)
    r = (used(out, ref_out, s_out, TOL_OUT), used(gm, ref_gm, s_gm, TOL_MASK),
         used(gf, ref_gf, s_gf, TOL_FLOW))
    print(f"{shape} {kind}: fraction of the bound used: out {r[0]:.3f}, grad_mask {r[1]:.3f}, "
          f"grad_flow {r[2]:.2e}")
    assert r[0] <= 1 and r[1] <= 1 and r[2] <= 1, r
    if kind == "neg_inf":
        assert (gm[mask == -np.inf] == 0).all()           # weight exactly 0


def test_graph_replay_equals_eager(dx):
    """Forward and backward captured in one single-stream graph after a warm-up
    call; replayed with new input contents."""
    shape = (2, 5, 67)
    mask, flow, gout = (dev(a) for a in inputs(shape))
    mask2, flow2, gout2 = (dev(a) for a in inputs(shape, "neg_inf"))
    m = mask.clone().requires_grad_()
    f = flow.clone().requires_grad_()
    g = gout.clone()
    state = {}

    def step():
        out = dx.upsample_flow(f, m)
        state["out"] = out
        state["gf"], state["gm"] = torch.autograd.grad(out, (f, m), g)

    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        step()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            step()
        for mm, ff, gg in ((mask2, flow2, gout2), (mask, flow, gout)):
            with torch.no_grad():
                m.copy_(mm)
                f.copy_(ff)
                g.copy_(gg)
                for t in state.values():
                    t.fill_(float("nan"))
            graph.replay()
            stream.synchronize()
            got = [state[k].clone() for k in ("out", "gf", "gm")]
            want = run(dx, mm, ff, gg)
            for a, b in zip(got, want):
                assert torch.equal(a, b)
    torch.cuda.synchronize()


def test_needs_input_grad_and_the_chain_through_the_flow(dx):
    shape = (2, 3, 1)
    mask, flow, gout = (dev(a) for a in inputs(shape))
    _, gf_ref, gm_ref = run(dx, mask, flow, gout)
    # flow = coords1 - coords0, the way the refinement loop forms it
    coords0 = torch.randn_like(flow)
    coords1 = (coords0 + flow).requires_grad_()
    m = mask.clone().requires_grad_()
    out = dx.upsample_flow(coords1 - coords0, m)
    out.backward(gout)
    _, gf_c, _ = run(dx, mask, coords1.detach() - coords0, gout)
    assert torch.equal(coords1.grad, gf_c) and coords0.grad is None
    # neither input requires grad: nothing is recorded
    assert not dx.upsample_flow(flow, mask).requires_grad
    # only the inputs are saved
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        f = flow.clone().requires_grad_()
        dx.upsample_flow(f, mask)
    assert len(saved) == 2 and {tuple(t.shape) for t in saved} == {tuple(flow.shape),
                                                                  tuple(mask.shape)}
    assert gf_ref is not None and gm_ref is not None


def test_double_backward_raises(dx):
    mask, flow, _ = (dev(a) for a in inputs((1, 1, 5)))
    f = flow.clone().requires_grad_()
    out = dx.upsample_flow(f, mask)
    # a loss whose grad_out depends on the input, so the first gradient has a history
    (g1,) = torch.autograd.grad(out.square().sum(), f, create_graph=True)
    assert g1.requires_grad
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g1.sum().backward()


def test_input_layouts_dtypes_and_empty_batch(dx):
    shape = (2, 5, 67)
    mask, flow, gout = (dev(a) for a in inputs(shape))
    ref = run(dx, mask, flow, gout)
    # a channels-last mask and a flow that is a view are copied to contiguous
    m_cl = mask.contiguous(memory_format=torch.channels_last)
    f_nc = flow.transpose(2, 3).contiguous().transpose(2, 3)
    assert not m_cl.is_contiguous() and not f_nc.is_contiguous()
    for a, b in zip(run(dx, m_cl, f_nc, gout), ref):
        assert torch.equal(a, b)
    # a 16-bit flow is widened
    f16 = flow.half()
    out16, gf16, _ = run(dx, mask, f16, gout)
    out32, gf32, _ = run(dx, mask, f16.float(), gout)
    assert torch.equal(out16, out32) and gf16.dtype == torch.float16
    assert torch.equal(gf16, gf32.half())
    # N == 0
    out = dx.upsample_flow(flow[:0], mask[:0])
    assert out.shape == (0, 2, 40, 536)


@pytest.mark.parametrize("shape", [(1, 1, 5), (2, 5, 67)])
def test_unaligned_pointers_take_the_scalar_path(dx, shape):
    """`out` and `grad_out` that are only 4-byte aligned: the kernels fall back from
    16-byte to 4-byte accesses and give the same bits."""
    from dexiraft_amd import _native as nat
    lib = nat.load()
    N, H, W = shape
    mask, flow, gout = (dev(a) for a in inputs(shape))
    out_ref, gf_ref, gm_ref = run(dx, mask, flow, gout)
    buf = torch.zeros(out_ref.numel() + 1, device=DEV)
    gbuf = torch.zeros(gout.numel() + 1, device=DEV)
    gbuf[1:] = gout.reshape(-1)
    gm, gf = torch.empty_like(mask), torch.empty_like(flow)
    nbytes = lib.dxu_convex_upsample_backward_workspace_bytes(N, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0 and gbuf.data_ptr() % 16 == 0
    stream = nat.stream_of(mask)
    nat.check(lib.dxu_convex_upsample(mask.data_ptr(), nat.DXU_MASK_F32, flow.data_ptr(), N, H, W,
                                      buf.data_ptr() + 4, stream), "forward")
    nat.check(lib.dxu_convex_upsample_backward(gbuf.data_ptr() + 4, mask.data_ptr(),
                                               nat.DXU_MASK_F32, flow.data_ptr(), N, H, W,
                                               gm.data_ptr(), gf.data_ptr(), ws.data_ptr(), nbytes,
                                               stream), "backward")
    torch.cuda.synchronize()
    assert torch.equal(buf[1:].view_as(out_ref), out_ref) and float(buf[0]) == 0.0
    assert torch.equal(gm, gm_ref) and torch.equal(gf, gf_ref)
