"""GPU: dexiraft_amd.forward_interpolate (csrc/flow_interp.hip, include/dexiraft_flow.h)
against a float64 brute force of its rule, and driver.infer_sequence's warm start.

The rule is fully specified (float64 landing positions, strict validity, d2 without
fused multiply-add, lowest source index among equal d2, copied bits), so equality
with the oracle below is ``torch.equal`` on every cell.  Against the REFERENCE's
recorded outputs (tests/golden/forward_interp.npz, scipy's KD-tree) equality is
asked at every grid point that is not near-tied: best and second-best d2, among
sources with a different flow value, further apart than a relative 1e-12; the
near-tied share is at most 1 % (asserted on the reference alone when the fixture
was made, tests/golden/make_forward_interp_golden.py).

Shapes: the search kernel works on tiles of 256 grid points and stages sources in
chunks of 256; a source slice is a whole number of chunks.  1x257 and 17x19 are
the smallest sizes past one tile and one slice that are a multiple of neither;
B = 512 at 17x19 makes the planner give each workgroup one slice of two chunks.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NEAR_TIE_REL = 1e-12
NEAR_TIE_CAP = 0.01


def oracle_forward_interpolate(flow: np.ndarray, want_near: bool = False, chunk: int = 1024):
    """The rule of include/dexiraft_flow.h in numpy float64, one item [2, H, W].

    Returns (out [2, H, W] float32, near [H, W] bool): ``near`` (filled when
    ``want_near``) marks grid points whose best and second-best d2 among sources
    with a different flow value agree to a relative NEAR_TIE_REL.  ``ex*ex +
    ey*ey`` is three separate ufunc calls: no fused multiply-add."""
    flow = np.ascontiguousarray(flow, dtype=np.float32)
    _, h, w = flow.shape
    n = h * w
    dx, dy = flow[0].reshape(-1), flow[1].reshape(-1)
    i = np.arange(n, dtype=np.int64)
    x0, y0 = i % w, i // w
    with np.errstate(invalid="ignore"):
        x1 = x0 + dx        # int64 + float32 -> float64, one addition
        y1 = y0 + dy
        valid = (x1 > 0) & (x1 < w) & (y1 > 0) & (y1 < h)
    assert x1.dtype == np.float64
    out = np.zeros((2, n), np.float32)
    near = np.zeros(n, bool)
    idx = np.flatnonzero(valid)            # ascending: argmin's first hit is the lowest index
    if idx.size:
        xs, ys, sdx, sdy = x1[idx], y1[idx], dx[idx], dy[idx]
        for g0 in range(0, n, chunk):
            g1 = min(n, g0 + chunk)
            ex = x0[g0:g1, None].astype(np.float64) - xs[None, :]
            ey = y0[g0:g1, None].astype(np.float64) - ys[None, :]
            xx = ex * ex
            yy = ey * ey
            d2 = xx + yy
            k = d2.argmin(axis=1)
            best = d2[np.arange(g1 - g0), k]
            out[0, g0:g1], out[1, g0:g1] = sdx[k], sdy[k]
            if not want_near:
                continue
            other = (sdx[None, :] != sdx[k][:, None]) | (sdy[None, :] != sdy[k][:, None])
            second = np.where(other, d2, np.inf).min(axis=1)
            fin = np.isfinite(second)
            near[g0:g1] = fin & (np.where(fin, second, 0.0) - best
                                 <= NEAR_TIE_REL * np.where(fin, second, 0.0))
    return out.reshape(2, h, w), near.reshape(h, w)


def gen_flow(seed: int, h: int, w: int) -> np.ndarray:
    """Continuous random flow, sigma min(3, size / 3) px per axis: most sources stay
    inside, some leave, even where an axis has one pixel."""
    rng = np.random.default_rng(seed)
    f = np.stack([rng.normal(0.0, min(3.0, w / 3.0), (h, w)),
                  rng.normal(0.0, min(3.0, h / 3.0), (h, w))])
    return f.astype(np.float32)


@lru_cache(maxsize=None)
def case(seed: int, h: int, w: int):
    """A generated flow and its oracle answer, computed once and shared (read-only)."""
    flow = gen_flow(seed, h, w)
    want, _ = oracle_forward_interpolate(flow)
    flow.setflags(write=False)
    want.setflags(write=False)
    return flow, want


def shape_case(h: int, w: int):
    return case(100 + h * 1000 + w, h, w)


def host(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.array(a))      # a copy: the shared cases are read-only


def dev(a: np.ndarray) -> torch.Tensor:
    return host(a).to(DEV)


@pytest.fixture(scope="module")
def dx():
    import dexiraft_amd
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    dexiraft_amd.load_native()
    return dexiraft_amd


def run(dx, flow: np.ndarray) -> torch.Tensor:
    out = dx.forward_interpolate(dev(flow))
    assert out.dtype == torch.float32 and out.is_contiguous() and out.device.type == "cuda"
    assert tuple(out.shape) == tuple(flow.shape)
    return out.cpu()


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("shape", ["6x8", "13x17", "24x40"])
def test_golden_inputs_match_oracle_and_reference(dx, shape):
    with np.load(GOLDEN / "forward_interp.npz") as z:
        flow, ref = z[f"flow_{shape}"], z[f"ref_{shape}"]
    want, near = oracle_forward_interpolate(flow, want_near=True)
    got = run(dx, flow)
    assert torch.equal(got, host(want))
    share = float(near.mean())
    print(f"{shape}: near-tied share {share:.4f}")
    assert share <= NEAR_TIE_CAP
    keep = host(~near)
    assert torch.equal(got[:, keep], host(ref)[:, keep])


@pytest.mark.parametrize("h,w", [(1, 1), (1, 9), (33, 1), (13, 17), (1, 257), (17, 19), (55, 128)])
def test_shapes_match_oracle(dx, h, w):
    flow, want = shape_case(h, w)
    assert torch.equal(run(dx, flow), host(want))


def test_one_pixel_image(dx):
    """1x1: the only source is valid iff it lands strictly inside (0, 1) x (0, 1)."""
    inside = np.array([0.5, 0.25], np.float32).reshape(2, 1, 1)
    assert torch.equal(run(dx, inside), host(inside))
    assert torch.equal(run(dx, np.zeros((2, 1, 1), np.float32)), torch.zeros(2, 1, 1))


def test_many_items_one_slice_of_two_chunks(dx):
    """B = 512 at 17x19: enough workgroups without splitting the sources, so every
    workgroup walks one slice of two LDS chunks (the second one partly filled)."""
    h, w, b = 17, 19, 512
    flows = np.stack([gen_flow(5000 + k, h, w) for k in range(b)])
    want = np.stack([oracle_forward_interpolate(f)[0] for f in flows])
    assert torch.equal(run(dx, flows), host(want))


def test_no_valid_source_gives_zeros(dx):
    flow = np.full((2, 9, 11), 1000.0, np.float32)
    assert torch.equal(run(dx, flow), torch.zeros(2, 9, 11))


def test_single_valid_source_fills_the_frame(dx):
    flow = np.full((2, 9, 11), 1000.0, np.float32)
    flow[:, 4, 6] = (0.5, -1.25)
    got = run(dx, flow)
    assert torch.equal(got[0], torch.full((9, 11), 0.5))
    assert torch.equal(got[1], torch.full((9, 11), -1.25))


def test_sources_on_the_border_are_excluded(dx):
    """x1 == 0, x1 == W, y1 == 0, y1 == H: the comparisons are strict."""
    h, w = 5, 7
    flow = np.full((2, h, w), 1000.0, np.float32)
    flow[:, 1, 2] = (-2.0, 0.25)     # x1 = 0
    flow[:, 1, 4] = (3.0, 0.25)      # x1 = 7 = W
    flow[:, 3, 1] = (0.25, -3.0)     # y1 = 0
    flow[:, 3, 5] = (0.25, 2.0)      # y1 = 5 = H
    flow[:, 4, 3] = (0.5, -0.5)      # the one valid source
    got = run(dx, flow)
    assert torch.equal(got[0], torch.full((h, w), 0.5))
    assert torch.equal(got[1], torch.full((h, w), -0.5))
    assert torch.equal(got, host(oracle_forward_interpolate(flow)[0]))


def test_nan_and_inf_sources_drop_out(dx):
    h, w = 13, 17
    base, _ = case(77, h, w)
    flow, far = base.copy(), base.copy()
    bad = [(0, 0, 0, np.nan), (1, 3, 5, np.nan), (0, 6, 16, np.inf), (1, 7, 2, -np.inf),
           (0, 12, 8, -np.inf), (1, 12, 16, np.inf)]
    for c, y, x, v in bad:
        flow[c, y, x] = v
        far[:, y, x] = 1000.0          # invalid by leaving the frame instead
    got = run(dx, flow)
    assert torch.isfinite(got).all()
    assert torch.equal(got, host(oracle_forward_interpolate(flow)[0]))
    assert torch.equal(got, run(dx, far))     # the rest is unchanged


def test_negative_zero_is_preserved(dx):
    flow = np.full((2, 5, 5), 1000.0, np.float32)
    flow[:, 2, 2] = (-0.0, 0.5)
    got = run(dx, flow)
    assert torch.signbit(got[0]).all() and (got[0] == 0).all()
    assert same_bits(got[0], torch.full((5, 5), -0.0))
    assert torch.equal(got[1], torch.full((5, 5), 0.5))


# (H, W, lower-index pixel (y, x), higher-index pixel (y, x), tied grid point (y, x)):
# the two sources land half a pixel left and right of the grid point, on its row.
# 17x19 puts them in different source slices (flat indices 5 and 300).
TIES = [(7, 8, (1, 1), (4, 5), (3, 3)), (17, 19, (0, 5), (15, 15), (8, 9))]


@pytest.mark.parametrize("h,w,lo,hi,at", TIES, ids=["7x8", "17x19-two-slices"])
def test_exact_ties_take_the_lowest_source_index(dx, h, w, lo, hi, at):
    def build(lo_side: float):
        """lo lands at (at.x + lo_side, at.y), hi at (at.x - lo_side, at.y)."""
        flow = np.full((2, h, w), 1000.0, np.float32)
        flow[:, lo[0], lo[1]] = (at[1] + lo_side - lo[1], at[0] - lo[0])
        flow[:, hi[0], hi[1]] = (at[1] - lo_side - hi[1], at[0] - hi[0])
        return flow
    for lo_side in (-0.5, 0.5):      # the second round swaps the two landing positions
        flow = build(lo_side)
        assert lo[0] * w + lo[1] < hi[0] * w + hi[1]
        assert not np.array_equal(flow[:, lo[0], lo[1]], flow[:, hi[0], hi[1]])
        got = run(dx, flow)
        assert torch.equal(got[:, at[0], at[1]], host(flow[:, lo[0], lo[1]]))
        # the whole column through the grid point is equidistant: all the lower index
        assert torch.equal(got[:, :, at[1]],
                           host(flow[:, lo[0], lo[1]])[:, None].expand(2, h))
        assert torch.equal(got, host(oracle_forward_interpolate(flow)[0]))


def test_batch_equals_single_calls(dx):
    h, w = 13, 17
    flows = np.stack([case(s, h, w)[0] for s in (77, 78, 79)])
    got = run(dx, flows)
    for k in range(3):
        assert torch.equal(got[k], run(dx, flows[k]))
        assert torch.equal(got[k], host(case(77 + k, h, w)[1]))


def test_non_contiguous_and_float16_inputs(dx):
    h, w = 13, 17
    big = dev(gen_flow(81, h, 2 * w))
    view = big[:, :, ::2]
    assert not view.is_contiguous()
    assert torch.equal(dx.forward_interpolate(view), dx.forward_interpolate(view.contiguous()))
    hwc = dev(case(77, h, w)[0]).permute(1, 2, 0).contiguous().permute(2, 0, 1)
    assert not hwc.is_contiguous()
    assert torch.equal(dx.forward_interpolate(hwc).cpu(), host(case(77, h, w)[1]))
    half = dev(case(77, h, w)[0]).half()
    got = dx.forward_interpolate(half)
    assert got.dtype == torch.float32
    assert torch.equal(got, dx.forward_interpolate(half.contiguous().float()))
    bf = dev(case(77, h, w)[0]).bfloat16()
    assert torch.equal(dx.forward_interpolate(bf), dx.forward_interpolate(bf.float()))


def test_two_runs_are_identical(dx):
    x = dev(shape_case(55, 128)[0])
    assert same_bits(dx.forward_interpolate(x), dx.forward_interpolate(x))


def test_non_default_stream(dx):
    x = dev(shape_case(17, 19)[0])
    eager = dx.forward_interpolate(x)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        got = dx.forward_interpolate(x)
    stream.synchronize()
    assert torch.equal(got, eager)


def test_graph_capture_on_one_stream(dx):
    """Captured on a single stream (no side streams, no parallel branches): the
    call neither synchronises nor copies to the host, and its workspace comes
    from the graph's pool.  The second replay reads new input contents."""
    a, b = dev(shape_case(17, 19)[0]), dev(gen_flow(82, 17, 19))
    ref_a, ref_b = dx.forward_interpolate(a), dx.forward_interpolate(b)
    x = a.clone()
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.no_grad(), torch.cuda.stream(stream):
        dx.forward_interpolate(x)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            out = dx.forward_interpolate(x)
        for src, ref in ((a, ref_a), (b, ref_b)):
            x.copy_(src)
            out.fill_(float("nan"))
            g.replay()
            stream.synchronize()
            assert torch.equal(out, ref)


class StubModel:
    """Stands in for RAFT(test_mode=True) with flow_init (core/raft.py:165-166,
    192-193): a fixed function of its inputs that records what it was given."""

    def __init__(self):
        self.inits, self.lows = [], []

    def __call__(self, a, b, iters=12, flow_init=None, test_mode=True):
        assert test_mode and a.shape[-2] % 8 == 0 and a.shape[-1] % 8 == 0
        self.inits.append(None if flow_init is None else flow_init.clone())
        flow = torch.stack([(a - b).mean(1)[0] * 3.0, (a * b - 0.25).mean(1)[0] * iters])[None]
        low = flow[..., ::8, ::8].contiguous()
        if flow_init is not None:
            assert flow_init.shape == low.shape
            low = low + 0.5 * flow_init
        self.lows.append(low.clone())
        return low, flow


def test_infer_sequence_warm_start(dx, tmp_path):
    g = torch.Generator().manual_seed(5)
    frames = torch.rand((4, 3, 20, 30), generator=g).to(DEV)
    paths = [tmp_path / f"frame{k:04d}.flo" for k in range(3)]
    model = StubModel()
    flows = dx.driver.infer_sequence(model, frames, iters=4, flo_paths=paths)
    assert flows.shape == (3, 2, 20, 30) and flows.dtype == torch.float32
    assert flows.device.type == "cuda"
    assert model.inits[0] is None
    for k in (1, 2):
        init = model.inits[k]
        assert init.is_cuda and init.shape == model.lows[k - 1].shape
        assert torch.equal(init, dx.forward_interpolate(model.lows[k - 1][0])[None])
    for k in range(3):
        np.testing.assert_array_equal(dx.driver.read_flo(paths[k]),
                                      flows[k].permute(1, 2, 0).cpu().numpy())
    cold = StubModel()
    flows_cold = dx.driver.infer_sequence(cold, frames, iters=4, warm_start=False)
    assert cold.inits == [None, None, None]
    assert torch.equal(flows_cold, flows)      # the stub's flow_up ignores flow_init
