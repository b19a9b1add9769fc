"""GPU: ``dexiraft_amd.sequence_loss`` / ``flow_metrics`` (csrc/flow_loss.hip,
reference train.py:48-73), forward and backward.

Shapes (B, H, W): one pixel; (2, 5, 7), H*W no multiple of 4, so the 4-byte path
with groups that straddle two items; (3, 16, 24), the 16-byte path; (2, 67, 131),
17554 pixels = 8 workgroups of 2048 and a ragged ninth, 4-byte path.  P in
{1, 3, 12, 32}.  Predictions are flow_gt + N(0, 2^2), about 20 % of the pixels
are invalid, about 3 % of flow_gt sit at or above max_flow = 400.

Tolerance tests: terms, loss and stats[1] within 1e-5 relative of the float64
oracle (tests/loss_oracle.py, pinned on the CPU by tests/test_seq_loss_cpu.py).
Derived, not measured: every summand is non-negative, so nothing cancels, and the
rounding budget is the subtraction, one add, a float32 chain of at most 16
additions plus a 6-level tree (the interface allows 64) and the final rounding:
about 70 * 2^-24 ~ 4e-6.  Each test prints the fraction of the bound used.

Exact tests (``torch.equal``): the five counts and every gradient element
against the float32 restatement of the oracle; determinism; the 4-byte path
against the 16-byte one; graph replay against eager.
"""
from __future__ import annotations

import ctypes
from functools import lru_cache

import numpy as np
import pytest
import torch

import loss_oracle as lo

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(1, 1, 1), (2, 5, 7), (3, 16, 24), (2, 67, 131)]
PS = [1, 3, 12, 32]
GAMMA, MAX_FLOW = 0.8, 400.0
TOL = 1e-5


@pytest.fixture(scope="module")
def dx():
    import dexiraft_amd
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    dexiraft_amd.load_native()
    return dexiraft_amd


@lru_cache(maxsize=None)
def inputs(shape, P=32, seed=0):
    """(preds, gt, valid) float32 numpy, read-only; the first P of the 32 predictions
    of a shape and seed."""
    if P != 32:
        preds, gt, valid = inputs(shape, 32, seed)
        return preds[:P], gt, valid
    B, H, W = shape
    rng = np.random.default_rng(1000 * seed + 100 * H + W + B)
    gt = rng.normal(0, 30, (B, 2, H, W)).astype(np.float32)
    big = rng.random((B, H, W)) < 0.03
    gt[:, 0][big] = 400.0                                   # mag == max_flow: excluded
    gt[:, 1][big] = rng.choice([0.0, 250.0], int(big.sum()))
    valid = (rng.random((B, H, W)) < 0.8).astype(np.float32)
    preds = tuple((gt + rng.normal(0, 2, gt.shape)).astype(np.float32) for _ in range(32))
    for a in (gt, valid, *preds):
        a.setflags(write=False)
    return preds, gt, valid


@lru_cache(maxsize=None)
def oracle(shape, P, seed=0):
    preds, gt, valid = inputs(shape, P, seed)
    return lo.sums64(preds, gt, valid, GAMMA, MAX_FLOW), lo.stats32(preds[-1], gt, valid, MAX_FLOW)


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def run(dx, preds, gt, valid, grad=True, scale=None, **kw):
    """(loss, terms, stats, grads) through the public function, without a host copy
    of the metrics; grads[i] is None where preds[i] does not require grad."""
    ps = [p.clone().requires_grad_(grad if isinstance(grad, bool) else grad[i])
          for i, p in enumerate(preds)]
    loss, m = dx.sequence_loss(ps, gt, valid, kw.pop("gamma", GAMMA), kw.pop("max_flow", MAX_FLOW),
                               sync_metrics=False)
    if loss.requires_grad:
        (loss if scale is None else loss * scale).backward()
    torch.cuda.synchronize()
    return loss.detach(), m["terms"], m["stats"], [p.grad for p in ps]


def used(got, ref):
    """|got - ref| / (TOL * |ref|) (0 when both are 0); the test passes when <= 1."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all()
    err, bound = np.abs(got - ref), TOL * np.abs(ref)
    return float(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300)).max())


@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("shape", SHAPES)
def test_sums_against_the_float64_oracle(dx, shape, P):
    preds, gt, valid = inputs(shape, P)
    (ref_loss, ref_terms, ref_epe), _ = oracle(shape, P)
    loss, terms, stats, _ = run(dx, [dev(p) for p in preds], dev(gt), dev(valid), grad=False)
    assert loss.dtype == terms.dtype == torch.float32 and stats.dtype == torch.float64
    assert loss.shape == () and terms.shape == (P,) and stats.shape == (6,)
    r = (used(terms.cpu().numpy(), ref_terms), used(float(loss), ref_loss),
         used(float(stats[1]), ref_epe))
    print(f"{shape} P={P}: fraction of the 1e-5 bound used: terms {r[0]:.3f}, loss {r[1]:.3f}, "
          f"sum epe {r[2]:.3f}")
    assert max(r) <= 1, r


@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("shape", SHAPES)
def test_counts_and_gradients_are_exact(dx, shape, P):
    preds, gt, valid = inputs(shape, P)
    _, counts = oracle(shape, P)
    _, _, stats, grads = run(dx, [dev(p) for p in preds], dev(gt), dev(valid))
    want = torch.tensor(counts, dtype=torch.float64, device=DEV)
    assert torch.equal(stats[[0, 2, 3, 4, 5]], want), (stats.tolist(), counts)
    for g, ref in zip(grads, lo.grads32(preds, gt, valid, GAMMA, MAX_FLOW)):
        assert g.dtype == torch.float32 and torch.equal(g, dev(ref))


def test_metrics_dict_is_the_reference_one(dx):
    shape, P = (2, 67, 131), 3
    preds, gt, valid = inputs(shape, P)
    (ref_loss, _, ref_epe), c = oracle(shape, P)
    loss, m = dx.sequence_loss([dev(p) for p in preds], dev(gt), dev(valid), GAMMA, MAX_FLOW)
    assert set(m) == {"epe", "1px", "3px", "5px"} and all(type(x) is float for x in m.values())
    assert used(float(loss), ref_loss) <= 1 and used(m["epe"], ref_epe / c[0]) <= 1
    assert (m["1px"], m["3px"], m["5px"]) == (c[1] / c[0], c[2] / c[0], c[3] / c[0])
    assert not loss.requires_grad
    # defaults are the reference's: gamma 0.8, max_flow 400
    loss2, m2 = dx.sequence_loss([dev(p) for p in preds], dev(gt), dev(valid))
    assert torch.equal(loss, loss2) and m == m2


def test_equal_prediction_has_zero_gradient_and_counts_below_one(dx):
    shape = (2, 5, 7)
    _, gt, _ = inputs(shape, 1)
    gt = np.array(gt)
    gt[gt == 400.0] = 1.0
    valid = np.ones((2, 5, 7), dtype=np.float32)
    pred = gt + np.float32(10.0)                           # epe = 14.1: no pixel below 5
    pred[1, :, 3, 4] = gt[1, :, 3, 4]
    pred[0, 0, 0, 0] = gt[0, 0, 0, 0]                      # dx == 0 only
    _, _, stats, (g,) = run(dx, [dev(pred)], dev(gt), dev(valid))
    assert stats.tolist()[0] == 70 and stats.tolist()[2:5] == [1, 1, 1]
    assert (g[1, :, 3, 4] == 0).all() and g[0, 0, 0, 0] == 0 and g[0, 1, 0, 0] > 0
    assert int((g == 0).sum()) == 3
    assert torch.equal(g, dev(lo.grads32([pred], gt, valid, GAMMA, MAX_FLOW)[0]))


def test_all_pixels_invalid(dx):
    shape, P = (3, 16, 24), 3
    preds, gt, _ = inputs(shape, P)
    zeros = torch.zeros(shape, device=DEV)
    loss, terms, stats, grads = run(dx, [dev(p) for p in preds], dev(gt), zeros)
    assert float(loss) == 0.0 and (terms == 0).all() and (stats == 0).all()
    assert all((g == 0).all() for g in grads)
    loss, m = dx.sequence_loss([dev(p) for p in preds], dev(gt), zeros)
    assert float(loss) == 0.0 and all(np.isnan(x) for x in m.values())
    # max_flow below every magnitude does the same
    loss, _, stats, _ = run(dx, [dev(p) for p in preds], dev(gt), None, grad=False, max_flow=0.0)
    assert float(loss) == 0.0 and (stats == 0).all()


def test_nan_prediction_at_an_invalid_pixel(dx):
    shape, P = (2, 5, 7), 3
    preds, gt, valid = inputs(shape, P)
    b, y, x = (int(i[0]) for i in np.nonzero(valid == 0))
    bad = np.array(preds[0])
    bad[b, 1, y, x] = np.nan
    (_, ref_terms, ref_epe), counts = oracle(shape, P)
    loss, terms, stats, _ = run(dx, [dev(bad), dev(preds[1]), dev(preds[2])], dev(gt), dev(valid),
                                grad=False)
    assert torch.isnan(loss) and torch.isnan(terms[0])
    assert used(terms[1:].cpu().numpy(), ref_terms[1:]) <= 1       # not the last: stats finite
    assert used(float(stats[1]), ref_epe) <= 1
    assert stats[[0, 2, 3, 4, 5]].tolist() == counts


@pytest.mark.parametrize("shape", SHAPES)
def test_flow_metrics_null_valid_and_infinite_max_flow(dx, shape):
    preds, gt, valid = inputs(shape, 1)
    pr, g = dev(preds[0]), dev(gt)
    s = dx.flow_metrics(pr, g)
    assert s.dtype == torch.float64 and s.shape == (6,) and s.device == pr.device
    assert torch.equal(s, dx.flow_metrics(pr, g, torch.ones(shape, device=DEV)))
    B, H, W = shape
    assert s.tolist()[0] == B * H * W
    assert s[[0, 2, 3, 4, 5]].tolist() == lo.stats32(preds[0], gt, None, float("inf"))
    assert used(float(s[1]), lo.sums64(preds, gt, None, 1.0, float("inf"))[2]) <= 1
    # the masked form is the statistics of sequence_loss, and a [2, H, W] flow is one item
    _, _, stats, _ = run(dx, [pr], g, dev(valid), grad=False)
    assert torch.equal(dx.flow_metrics(pr, g, dev(valid), MAX_FLOW), stats)
    assert torch.equal(dx.flow_metrics(pr[0], g[0], dev(valid)[0], MAX_FLOW),
                       dx.flow_metrics(pr[:1], g[:1], dev(valid)[:1], MAX_FLOW))


def test_one_tensor_as_several_predictions_gets_the_sum(dx):
    shape = (3, 16, 24)
    preds, gt, valid = inputs(shape, 3)
    g, v = dev(gt), dev(valid)
    x = dev(preds[0]).requires_grad_()
    loss, _ = dx.sequence_loss([x, x, x], g, v, sync_metrics=False)
    loss.backward()
    _, _, _, grads = run(dx, [x.detach()] * 3, g, v)
    want = grads[0].double() + grads[1].double() + grads[2].double()
    assert (x.grad.double() - want).abs().max() <= 2.0 ** -22 * want.abs().max()
    assert torch.equal(x.grad == 0, grads[0] == 0)


def test_only_some_predictions_require_grad(dx):
    shape, P = (2, 67, 131), 3
    preds, gt, valid = inputs(shape, P)
    ps, g, v = [dev(p) for p in preds], dev(gt), dev(valid)
    _, _, _, full = run(dx, ps, g, v)
    loss, _, _, some = run(dx, ps, g, v, grad=[True, False, True])
    assert some[1] is None and torch.equal(some[0], full[0]) and torch.equal(some[2], full[2])
    assert not run(dx, ps, g, v, grad=False)[0].requires_grad
    # only references to the inputs are saved
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        q = [p.clone().requires_grad_() for p in ps]
        dx.sequence_loss(q, g, v, sync_metrics=False)
    assert {t.data_ptr() for t in saved} == {t.data_ptr() for t in (*q, g, v)}
    # the C-ABI writes nothing for a null entry of grad_preds
    from dexiraft_amd import _native as nat
    lib = nat.load()
    B, H, W = shape
    out = [torch.empty_like(ps[0]), None, torch.empty_like(ps[2])]
    one = torch.ones((), device=DEV)
    arr = lambda ts: (ctypes.c_void_p * len(ts))(*[nat.ptr(t) for t in ts])   # noqa: E731
    nat.check(lib.dxl_sequence_loss_backward(one.data_ptr(), arr(ps), arr(out), P, g.data_ptr(),
                                             v.data_ptr(), B, H, W, GAMMA, MAX_FLOW,
                                             nat.stream_of(g)), "backward")
    torch.cuda.synchronize()
    assert torch.equal(out[0], full[0]) and torch.equal(out[2], full[2])


@pytest.mark.parametrize("shape", [(2, 5, 7), (3, 16, 24)])
def test_scaled_loss(dx, shape):
    P, scale = 3, 3.7
    preds, gt, valid = inputs(shape, P)
    _, _, _, grads = run(dx, [dev(p) for p in preds], dev(gt), dev(valid), scale=scale)
    for g, ref in zip(grads, lo.grads32(preds, gt, valid, GAMMA, MAX_FLOW, scale)):
        assert torch.equal(g, dev(ref))


@pytest.mark.parametrize("shape", SHAPES)
def test_two_runs_are_bit_equal(dx, shape):
    preds, gt, valid = inputs(shape, 12, seed=1)
    a = run(dx, [dev(p) for p in preds], dev(gt), dev(valid))
    b = run(dx, [dev(p) for p in preds], dev(gt), dev(valid))
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x, y)
    for x, y in zip(a[3], b[3]):
        assert torch.equal(x, y)


def test_misaligned_pointers_take_the_scalar_path(dx):
    """A prediction and a gradient buffer that are only 4-byte aligned: the kernels
    fall back from 16-byte to 4-byte accesses and give the same bits."""
    from dexiraft_amd import _native as nat
    lib = nat.load()
    shape, P = (3, 16, 24), 3
    B, H, W = shape
    preds, gt, valid = inputs(shape, P)
    ps, g, v = [dev(p) for p in preds], dev(gt), dev(valid)
    loss_ref, terms_ref, stats_ref, grads_ref = run(dx, ps, g, v)
    n = ps[0].numel()
    pbuf = torch.zeros(n + 1, device=DEV)
    pbuf[1:] = ps[1].reshape(-1)
    gbuf = torch.full((n + 2,), 7.0, device=DEV)
    assert pbuf.data_ptr() % 16 == 0 and gbuf.data_ptr() % 16 == 0
    arr = lambda xs: (ctypes.c_void_p * len(xs))(*xs)   # noqa: E731
    pp = arr([ps[0].data_ptr(), pbuf.data_ptr() + 4, ps[2].data_ptr()])
    loss, terms = torch.empty((), device=DEV), torch.empty(P, device=DEV)
    stats = torch.empty(6, dtype=torch.float64, device=DEV)
    nbytes = lib.dxl_sequence_loss_workspace_bytes(P, B, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    stream = nat.stream_of(g)
    nat.check(lib.dxl_sequence_loss(pp, P, g.data_ptr(), v.data_ptr(), B, H, W, GAMMA, MAX_FLOW,
                                    loss.data_ptr(), terms.data_ptr(), stats.data_ptr(),
                                    ws.data_ptr(), nbytes, stream), "forward")
    out = [torch.empty_like(p) for p in ps]
    gp = arr([out[0].data_ptr(), out[1].data_ptr(), gbuf.data_ptr() + 4])
    one = torch.ones((), device=DEV)
    nat.check(lib.dxl_sequence_loss_backward(one.data_ptr(), pp, gp, P, g.data_ptr(), v.data_ptr(),
                                             B, H, W, GAMMA, MAX_FLOW, stream), "backward")
    torch.cuda.synchronize()
    assert torch.equal(loss, loss_ref) and torch.equal(terms, terms_ref)
    assert torch.equal(stats, stats_ref)
    assert torch.equal(out[0], grads_ref[0]) and torch.equal(out[1], grads_ref[1])
    assert torch.equal(gbuf[1:-1].view_as(ps[2]), grads_ref[2])
    assert float(gbuf[0]) == 7.0 and float(gbuf[-1]) == 7.0


def test_graph_replay_equals_eager(dx):
    """Forward and backward captured in one single-stream graph after a warm-up
    call (sync_metrics=False: no host copy); replayed with new input contents."""
    shape, P = (2, 67, 131), 3
    sets = [inputs(shape, P, seed) for seed in (0, 1)]
    ps = [dev(p).requires_grad_() for p in sets[0][0]]
    g, v = dev(sets[0][1]), dev(sets[0][2])
    scale = torch.tensor(2.5, device=DEV)
    state = {}

    def step():
        loss, m = dx.sequence_loss(ps, g, v, GAMMA, MAX_FLOW, sync_metrics=False)
        state["loss"], state["terms"], state["stats"] = loss, m["terms"], m["stats"]
        state["g0"], state["g1"], state["g2"] = torch.autograd.grad(loss * scale, ps)

    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        step()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            step()
        for preds, gt, valid in (sets[1], sets[0]):
            with torch.no_grad():
                for t, a in zip(ps, preds):
                    t.copy_(dev(a))
                g.copy_(dev(gt))
                v.copy_(dev(valid))
                for t in state.values():
                    t.fill_(float("nan"))
            graph.replay()
            stream.synchronize()
            got = [state[k].clone() for k in ("loss", "terms", "stats", "g0", "g1", "g2")]
            loss, terms, stats, grads = run(dx, [dev(a) for a in preds], dev(gt), dev(valid),
                                            scale=2.5)
            for a, b in zip(got, (loss, terms, stats, *grads)):
                assert torch.equal(a, b)
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape,P", [((2, 5, 7), 3), ((2, 67, 131), 12)])
def test_agrees_with_the_torch_sequence_on_the_gpu(dx, shape, P):
    """The torch ops of the definition on the same GPU: the loss to 1e-5 relative,
    every gradient element to 2 ulp, the counts exactly."""
    preds, gt, valid = inputs(shape, P)
    g, v = dev(gt), dev(valid)
    loss, _, stats, grads = run(dx, [dev(p) for p in preds], g, v)
    tp = [dev(p).requires_grad_() for p in preds]
    tl, ts = lo.torch_sequence(tp, g, v, GAMMA, MAX_FLOW)
    tl.backward()
    tl, ts = tl.detach(), ts.detach()
    assert abs(float(loss) - float(tl)) <= TOL * abs(float(tl))
    assert torch.equal(stats[[0, 2, 3, 4]], ts[[0, 2, 3, 4]])
    assert abs(float(stats[1]) - float(ts[1])) <= TOL * float(ts[1])
    for a, t in zip(grads, tp):
        assert ((a - t.grad).abs() <= 2 * 2.0 ** -23 * t.grad.abs()).all()


def test_double_backward_raises_and_inputs_are_converted(dx):
    shape, P = (2, 5, 7), 3
    preds, gt, valid = inputs(shape, P)
    ps, g, v = [dev(p) for p in preds], dev(gt), dev(valid)
    loss_ref, _, stats_ref, grads_ref = run(dx, ps, g, v)
    x = ps[0].clone().requires_grad_()
    loss, _ = dx.sequence_loss([x, ps[1], ps[2]], g, v, sync_metrics=False)
    (g1,) = torch.autograd.grad(loss * loss, x, create_graph=True)
    assert g1.requires_grad
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g1.sum().backward()
    # a non-contiguous prediction, a float64 flow_gt and a bool valid are converted first
    nc = ps[0].transpose(2, 3).contiguous().transpose(2, 3).requires_grad_()
    assert not nc.is_contiguous()
    loss, m = dx.sequence_loss([nc, ps[1], ps[2]], g.double(), v.bool(), sync_metrics=False)
    loss.backward()
    assert torch.equal(loss.detach(), loss_ref) and torch.equal(m["stats"], stats_ref)
    assert torch.equal(nc.grad, grads_ref[0])
    # a float16 prediction is widened; its gradient comes back through the conversion
    h = ps[0].half().requires_grad_()
    loss16, _ = dx.sequence_loss([h, ps[1], ps[2]], g, v, sync_metrics=False)
    loss16.backward()
    want = run(dx, [h.detach().float(), ps[1], ps[2]], g, v)
    assert torch.equal(loss16.detach(), want[0]) and h.grad.dtype == torch.float16
    assert torch.equal(h.grad, want[3][0].half())
