"""GPU: training through the on-the-fly block (TrainableAlternateCorrBlock and
``dxr_alt_corr_backward`` with DXR_ALT_BWD_ACCUMULATE) against a float64 oracle
of the whole block.

The oracle is composed here from the pinned pieces: per level
``oracle.alt_corr_backward`` on (fmap1, the float64-pooled fmap2 level,
coords / 2^l in float32, that level's channel slice of grad_out), the fmap2
level gradients folded with ``oracle.avg_pool2x2_backward``, and the 1/sqrt(D)
scale.  ``M`` is the same composition on |fmap1|, |fmap2|, |grad_out| (the
bilinear weights are non-negative).

Per element the rule of
tests/test_gpu_alt_oracle.py::test_alt_backward_matches_oracle_per_element
applies: |got - ref| <= 4 n 2^-24 M with n that element's own number of
contributions — for dfmap1 the on-map window cells of the query over all
lookups and levels, for dfmap2 the per-level counts of (lookup, query, window
cell) landing on a cell, folded up with the pooling footprint — plus
num_levels + 2 for the fold and the scale.  An element with M == 0 is exactly 0
and everything is finite.  Every run prints the observed max err / M.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest
import torch

import datagen as dg
import oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
F32 = np.float32


@pytest.fixture(scope="module")
def dx():
    import dexiraft_amd
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    dexiraft_amd.load_native()
    return dexiraft_amd


def _t(a: np.ndarray, **kw) -> torch.Tensor:
    return torch.from_numpy(np.array(a)).to(DEV, **kw)


# name -> (B, D, H, W, L, r, K lookups, coordinate model)
CASES = {
    "ragged": (2, 48, 18, 21, 4, 4, 3, "normal3"),      # ragged tiles, remainders at 9 -> 4
    "uniform": (2, 48, 18, 21, 4, 4, 2, "uniform6"),    # whole-level boxes, windows off every side
    "d256": (1, 256, 16, 24, 4, 4, 2, "normal4"),
    "small": (1, 128, 16, 16, 4, 3, 2, "normal4"),      # the small model
    "tiles": (1, 80, 44, 48, 4, 4, 1, "normal4"),       # more tiles than XCDs, 5 k-blocks
    "r0": (1, 16, 16, 16, 4, 0, 1, "normal4"),
    "r6": (1, 16, 16, 16, 4, 6, 1, "normal4"),
    "d36": (2, 36, 18, 21, 4, 4, 1, "normal3"),         # the fallback: the library declines
}


def _seed(name: str) -> int:
    return 7000 + 97 * list(CASES).index(name)


def _coords(seed, B, H, W, model):
    if model == "normal3":
        return dg.coords(seed, B, H, W, "normal", 3.0)
    if model == "normal4":
        return dg.coords(seed, B, H, W, "normal", 4.0)
    assert model == "uniform6"
    u = dg.uniform(seed, B * 2 * H * W).reshape(B, 2, H, W)
    c = u * np.array([W + 12.0, H + 12.0]).reshape(1, 2, 1, 1) - 6.0
    return c.astype(F32)


@lru_cache(maxsize=None)
def case_inputs(name: str, variant: str = ""):
    """(f1, f2 [B, D, H, W], coords list, grad_out list): read-only float32 arrays.
    variants: "sparse" (one lookup, grad_out non-zero in one channel per query),
    "nonfinite" (NaN, +-inf and 1e30 poked into a few queries' coords), "one"
    (the first lookup only)."""
    B, D, H, W, L, r, K, model = CASES[name]
    sd = _seed(name)
    C = L * (2 * r + 1) ** 2
    f1, f2 = dg.fmap(sd, B, D, H, W), dg.fmap(sd + 1, B, D, H, W)
    if variant in ("sparse", "one"):
        K = 1
    cs = [_coords(sd + 10 + k, B, H, W, model) for k in range(K)]
    gs = [dg.fmap(sd + 30 + k, B, C, H, W) for k in range(K)]
    if variant == "sparse":
        q = np.arange(H * W).reshape(H, W)
        keep = (np.arange(C)[:, None, None] == (q % C)[None])
        gs = [np.where(keep[None], g, F32(0)) for g in gs]
        assert keep.any(axis=(1, 2)).all()           # every channel is hit
    if variant == "nonfinite":
        for c in cs:
            c[0, 0, 3, 5] = np.nan
            c[0, 1, 7, 7] = np.inf
            c[0, 0, 0, 0] = -np.inf
            c[0, :, 2, 2] = 1e30
            c[1, 1, 10, 2:20:3] = -1e30
            c[1, :, 17, 20] = np.nan
    for a in [f1, f2] + cs + gs:
        a.setflags(write=False)
    return f1, f2, cs, gs


def _floor_index(v: np.ndarray) -> np.ndarray:
    """floor as int64; NaN, +-inf and huge values get a cell off every level."""
    with np.errstate(invalid="ignore"):
        f = np.floor(v)
        ok = np.abs(f) < 2.0 ** 40
    return np.where(ok, f, -2.0 ** 40).astype(np.int64)


def _counts(c_l: np.ndarray, r: int, H2: int, W2: int):
    """(per query [B, H, W] number of on-map window cells, per cell [B, H2, W2]
    number of (query, window cell) pairs landing on it) of one level's coords
    [B, H, W, 2]."""
    B = c_l.shape[0]
    x0 = _floor_index(c_l[..., 0]).reshape(B, -1)
    y0 = _floor_index(c_l[..., 1]).reshape(B, -1)
    per_q = np.zeros(x0.shape, dtype=np.int64)
    per_c = np.zeros((B, H2, W2), dtype=np.int64)
    for iy in range(2 * r + 2):
        for ix in range(2 * r + 2):
            h2, w2 = y0 - r + iy, x0 - r + ix
            ok = (h2 >= 0) & (h2 < H2) & (w2 >= 0) & (w2 < W2)
            per_q += ok
            for b in range(B):
                np.add.at(per_c[b], (h2[b][ok[b]], w2[b][ok[b]]), 1)
    return per_q.reshape(c_l.shape[:3]), per_c


def _unpool(a: np.ndarray, shape) -> np.ndarray:
    """The pooling footprint: each coarse cell's value on its 2 x 2 fine cells, 0 on
    the floor-mode remainder (a is [..., Ho, Wo])."""
    out = np.zeros(a.shape[:-2] + tuple(shape), dtype=a.dtype)
    Ho, Wo = a.shape[-2:]
    for i in range(2):
        for j in range(2):
            out[..., i:2 * Ho:2, j:2 * Wo:2] = a
    return out


def block_oracle(f1, f2, cs, gs, L, r, absolute=False):
    """float64 (dfmap1, dfmap2) [B, D, H, W] of sum_k <lookup_k(coords_k), grad_out_k>."""
    B, D, H, W = f1.shape
    rr = (2 * r + 1) ** 2
    ab = np.abs if absolute else (lambda a: a)
    a1 = ab(f1.astype(np.float64)).transpose(0, 2, 3, 1)
    levels = [ab(f2.astype(np.float64))]
    for _ in range(1, L):
        levels.append(oracle.avg_pool2x2(levels[-1]))
    d1 = np.zeros((B, H, W, D))
    d2 = [np.zeros(lv.shape[:1] + lv.shape[2:] + (D,)) for lv in levels]
    for c, g in zip(cs, gs):
        cq = np.asarray(c, dtype=F32).transpose(0, 2, 3, 1)
        for l in range(L):
            c_l = (cq / F32(2 ** l)).reshape(B, 1, H, W, 2)
            g_l = ab(g[:, l * rr:(l + 1) * rr].astype(np.float64)).reshape(B, 1, rr, H, W)
            with np.errstate(invalid="ignore"):
                e1, e2, _ = oracle.alt_corr_backward(a1, levels[l].transpose(0, 2, 3, 1), c_l, g_l, r)
            d1 += e1
            d2[l] += e2
    tot = d2[L - 1].transpose(0, 3, 1, 2)
    for l in range(L - 2, -1, -1):
        tot = d2[l].transpose(0, 3, 1, 2) + oracle.avg_pool2x2_backward(tot, levels[l].shape[-2:])
    s = np.float64(np.sqrt(F32(D), dtype=F32))
    return d1.transpose(0, 3, 1, 2) / s, tot / s


def contributions(shape, cs, L, r):
    """(n1 [B, 1, H, W], n2 [B, 1, H, W]): the counted contributions per element."""
    B, D, H, W = shape
    sizes = [(H, W)]
    for _ in range(1, L):
        sizes.append((sizes[-1][0] // 2, sizes[-1][1] // 2))
    n1 = np.zeros((B, H, W), dtype=np.int64)
    per = [np.zeros((B,) + s, dtype=np.int64) for s in sizes]
    for c in cs:
        cq = np.asarray(c, dtype=F32).transpose(0, 2, 3, 1)
        for l in range(L):
            q, cell = _counts(cq / F32(2 ** l), r, *sizes[l])
            n1 += q
            per[l] += cell
    tot = per[L - 1]
    for l in range(L - 2, -1, -1):
        tot = per[l] + _unpool(tot, sizes[l])
    return n1[:, None] + (L + 2), tot[:, None] + (L + 2)


def _zero_dropped(cs, gs):
    """grad_out with the queries of a NaN / infinite coordinate zeroed."""
    out = []
    for c, g in zip(cs, gs):
        bad = ~np.isfinite(c).all(axis=1, keepdims=True)
        out.append(np.where(bad, F32(0), g))
    return out


@lru_cache(maxsize=None)
def reference(name: str, variant: str = ""):
    f1, f2, cs, gs = case_inputs(name, variant)
    B, D, H, W, L, r, K, model = CASES[name]
    go = _zero_dropped(cs, gs) if variant == "nonfinite" else gs
    ref = block_oracle(f1, f2, cs, go, L, r)
    M = block_oracle(f1, f2, cs, go, L, r, absolute=True)
    n = contributions(f1.shape, cs, L, r)
    for a in ref + M + n:
        a.setflags(write=False)
    return ref, M, n


def check(label, got, ref, M, n, extra=(0.0, 0.0)):
    """got: (dfmap1, dfmap2) arrays or None; the per-element rule of the module
    docstring (``extra``: an allowance in units of M added to the bound)."""
    for name, g, rf, m, cnt, ex in zip(("dfmap1", "dfmap2"), got, ref, M, n, extra):
        if g is None:
            continue
        g = np.asarray(g, dtype=np.float64)
        assert g.shape == rf.shape
        assert np.isfinite(g).all(), f"{label} {name}: non-finite gradient"
        err = np.abs(g - rf)
        bound = (4.0 * cnt * U + ex) * m
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(m > 0, err / m, 0.0)
            worst = np.where(m > 0, err / np.where(bound > 0, bound, 1.0), 0.0).max()
        print(f"ALT-TRAIN {label} {name}: max |err| / M {rel.max():.3e}, worst err / bound "
              f"{worst:.3e} (contributions {int(cnt.min())}..{int(cnt.max())})")
        assert (m > 0).any()
        assert not g[m == 0].any(), f"{label} {name}: an element with M == 0 is not exactly 0"
        assert (err <= bound).all(), f"{label} {name}: {int((err > bound).sum())} elements out"


def run_block(dx, name, variant="", cls=None, needs=(True, True), dtype=torch.float32, **kw):
    """Gradients of sum_k <block(coords_k), grad_out_k> through the block."""
    f1, f2, cs, gs = case_inputs(name, variant)
    B, D, H, W, L, r, K, model = CASES[name]
    t1 = _t(f1, dtype=dtype).requires_grad_(needs[0])
    t2 = _t(f2, dtype=dtype).requires_grad_(needs[1])
    blk = (cls or dx.TrainableAlternateCorrBlock)(t1, t2, L, r, **kw)
    outs = [blk(_t(c)) for c in cs]
    wanted = [t for t, nd in zip((t1, t2), needs) if nd]
    return blk, outs, wanted, [_t(g) for g in gs]


def grads_of(outs, wanted, gouts, needs=(True, True), **kw):
    gr = list(torch.autograd.grad(outs, wanted, [g.to(o.dtype) for g, o in zip(gouts, outs)], **kw))
    torch.cuda.synchronize()
    return tuple(gr.pop(0).cpu().numpy() if nd else None for nd in needs)


@pytest.mark.parametrize("name", ["ragged", "uniform", "d256", "small", "tiles", "r0", "r6"])
def test_block_gradients_match_the_float64_oracle(dx, name):
    ref, M, n = reference(name)
    blk, outs, wanted, gouts = run_block(dx, name)
    assert blk._bwd_native
    got = grads_of(outs, wanted, gouts)
    assert blk._bwd_native, "the library declined the accumulate flag"
    assert all(g.shape == case_inputs(name)[0].shape for g in got)
    check(name, got, ref, M, n)


def test_sparse_taps(dx):
    """One non-zero grad_out channel per query, every channel hit: each dfmap1 row
    has at most 4 contributions, so a dropped or misplaced tap shows."""
    ref, M, n = reference("ragged", "sparse")
    L = CASES["ragged"][4]
    # one tap feeds at most 4 window cells: that, not the window, bounds a dfmap1 row here
    n = (np.minimum(n[0], 4 + L + 2), n[1])
    blk, outs, wanted, gouts = run_block(dx, "ragged", "sparse")
    check("sparse", grads_of(outs, wanted, gouts), ref, M, n)


def test_nonfinite_coordinates_contribute_nothing(dx):
    ref, M, n = reference("ragged", "nonfinite")
    blk, outs, wanted, gouts = run_block(dx, "ragged", "nonfinite")
    check("nonfinite", grads_of(outs, wanted, gouts), ref, M, n)


def test_fallback_for_other_channel_counts(dx):
    """D = 36: the library declines the flag; the unflagged call plus torch adds."""
    ref, M, n = reference("d36")
    blk, outs, wanted, gouts = run_block(dx, "d36")
    got = grads_of(outs, wanted, gouts)
    assert not blk._bwd_native
    check("d36 fallback", got, ref, M, n)


def test_only_fmap1_requires_grad(dx):
    ref, M, n = reference("ragged", "one")
    blk, outs, wanted, gouts = run_block(dx, "ragged", "one", needs=(True, False))
    assert len(wanted) == 1
    check("fmap1 only", grads_of(outs, wanted, gouts, needs=(True, False)), ref, M, n)
    blk, outs, wanted, gouts = run_block(dx, "ragged", "one", needs=(False, True))
    check("fmap2 only", grads_of(outs, wanted, gouts, needs=(False, True)), ref, M, n)


def test_retain_graph_and_a_second_backward(dx):
    ref, M, n = reference("ragged", "one")
    blk, outs, wanted, gouts = run_block(dx, "ragged", "one")
    first = grads_of(outs, wanted, gouts, retain_graph=True)
    second = grads_of(outs, wanted, gouts)
    check("first backward", first, ref, M, n)
    check("second backward", second, ref, M, n)
    assert np.array_equal(first[0], second[0])      # dfmap1 has a fixed summation order


def test_no_grad_outputs_are_the_parents_bit_for_bit(dx):
    f1, f2, cs, gs = case_inputs("ragged", "one")
    B, D, H, W, L, r, K, model = CASES["ragged"]
    c = _t(cs[0])
    want = dx.AlternateCorrBlock(_t(f1), _t(f2), L, r)(c)
    t1, t2 = _t(f1).requires_grad_(True), _t(f2).requires_grad_(True)
    with torch.no_grad():
        a = dx.TrainableAlternateCorrBlock(t1, t2, L, r)(c)
    b = dx.TrainableAlternateCorrBlock(_t(f1), _t(f2), L, r)(c)          # nothing requires grad
    blk = dx.TrainableAlternateCorrBlock(t1, t2, L, r)
    with torch.no_grad():
        d = blk(c)
    e = blk(c)                                                           # under grad: same forward
    for o in (a, b, d):
        assert o.grad_fn is None and not o.requires_grad
        assert torch.equal(o, want)
    assert e.grad_fn is not None and torch.equal(e.detach(), want)
    with pytest.raises(NotImplementedError):
        blk(c.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError):      # the parent is as it was
        dx.AlternateCorrBlock(t1, t2, L, r)


def test_out_dtype_and_memory_format_under_grad(dx):
    """float16 channels-last outputs: the same gradients as the float32 NCHW loss
    on .float() outputs (grad_out arrives as float16 channels-last; its values
    are float16-representable here, so both losses have the same gradient)."""
    f1, f2, cs, gs = case_inputs("ragged", "one")
    B, D, H, W, L, r, K, model = CASES["ragged"]
    g16 = _t(gs[0]).half()
    gq = [g16.float().cpu().numpy()]
    ref = block_oracle(f1, f2, cs, gq, L, r)
    M = block_oracle(f1, f2, cs, gq, L, r, absolute=True)
    n = contributions(f1.shape, cs, L, r)
    blk, outs, wanted, _ = run_block(dx, "ragged", "one", out_dtype=torch.float16,
                                     memory_format=torch.channels_last)
    o = outs[0]
    assert o.dtype == torch.float16 and o.is_contiguous(memory_format=torch.channels_last)
    plain = dx.AlternateCorrBlock(_t(f1), _t(f2), L, r, out_dtype=torch.float16,
                                  memory_format=torch.channels_last)(_t(cs[0]))
    assert torch.equal(o.detach(), plain)
    got = grads_of(outs, wanted, [g16.contiguous(memory_format=torch.channels_last)])
    check("f16 channels-last", got, ref, M, n)
    blk2, outs2, wanted2, _ = run_block(dx, "ragged", "one")
    got2 = grads_of([outs2[0].float()], wanted2, [g16.float()])
    assert np.array_equal(got[0], got2[0])          # dfmap1: fixed order, the same taps
    check("f32 NCHW, same loss", got2, ref, M, n)


def test_bf16_fmaps_get_bf16_gradients(dx):
    f1, f2, cs, gs = case_inputs("ragged", "one")
    B, D, H, W, L, r, K, model = CASES["ragged"]
    blk, outs, wanted, gouts = run_block(dx, "ragged", "one", dtype=torch.bfloat16)
    g = torch.autograd.grad(outs, wanted, gouts)
    assert all(t.dtype == torch.bfloat16 and t.shape == (B, D, H, W) for t in g)
    # the float32 gradients of the widened values, cast
    w1 = wanted[0].detach().float().requires_grad_(True)
    w2 = wanted[1].detach().float().requires_grad_(True)
    blk32 = dx.TrainableAlternateCorrBlock(w1, w2, L, r)
    assert torch.equal(blk32(_t(cs[0])).detach(), outs[0].detach())
    g32 = torch.autograd.grad([blk32(_t(cs[0]))], [w1, w2], gouts)
    assert torch.equal(g[0], g32[0].to(torch.bfloat16))      # dfmap1: fixed summation order
    # against the oracle of the widened values
    wf1, wf2 = w1.detach().cpu().numpy(), w2.detach().cpu().numpy()
    ref = block_oracle(wf1, wf2, cs, gs, L, r)
    M = block_oracle(wf1, wf2, cs, gs, L, r, absolute=True)
    n = contributions(wf1.shape, cs, L, r)
    # dfmap2's float32 value moves within its bound with the atomics' order (two runs: twice
    # the bound apart), and the cast rounds to nearest: half a bfloat16 step, 2^-8 relative
    a, b = g[1].float().cpu().numpy().astype(np.float64), g32[1].cpu().numpy().astype(np.float64)
    apart = 2 * 4.0 * n[1] * U * M[1]
    assert (np.abs(a - b) <= 2.0 ** -8 * (np.abs(b) + apart) + apart).all()
    check("bf16 (widened)", tuple(t.cpu().numpy() for t in g32), ref, M, n)


def test_agrees_with_the_trainable_pyramid_block(dx):
    """CorrBlock and TrainableAlternateCorrBlock are the same function of the fmaps
    (SURVEY a7), so their gradients for the same loss agree within the sum of
    their bounds.  CorrBlock's: the same counted contributions (its GEMMs add
    exact zeros elsewhere) at 4 n 2^-24 M, plus 2^-21 M for its f16-pair
    operand split (the dropped lo x lo products, 2^-22, and the rounding of lo)."""
    ref, M, n = reference("ragged")
    blk, outs, wanted, gouts = run_block(dx, "ragged")
    alt = grads_of(outs, wanted, gouts)
    blk, outs, wanted, gouts = run_block(dx, "ragged", cls=dx.CorrBlock)
    pyr = grads_of(outs, wanted, gouts)
    for name, a, p, m, cnt in zip(("dfmap1", "dfmap2"), alt, pyr, M, n):
        bound = (2 * 4.0 * cnt * U + 2.0 ** -21) * m
        err = np.abs(a.astype(np.float64) - p)
        with np.errstate(divide="ignore", invalid="ignore"):
            print(f"ALT-TRAIN vs CorrBlock {name}: max |diff| / M "
                  f"{np.where(m > 0, err / m, 0.0).max():.3e}")
        assert (err <= bound).all()
    check("CorrBlock itself", pyr, ref, M, n, extra=(2.0 ** -21, 2.0 ** -21))


def test_capi_flagged_call_adds_on_top(dx):
    """A flagged call into sentinel-prefilled gradient buffers adds exactly on top
    (prefilled minus sentinel matches the zero-filled call within the bounds) and
    the guard floats behind both buffers keep their bits; Nc = 2 coordinate sets
    (fmap1_grad by atomics)."""
    from dexiraft_amd import _native as nat
    lib = nat.load()
    B, H1, W1, H2, W2, C, Nc, r = 2, 9, 13, 7, 11, 48, 2, 2
    rr, sd, GUARD, SENT = (2 * r + 1) ** 2, 9100, 4096, 1.5
    f1 = dg.normal(sd, B * H1 * W1 * C).reshape(B, H1, W1, C).astype(F32)
    f2 = dg.normal(sd + 1, B * H2 * W2 * C).reshape(B, H2, W2, C).astype(F32)
    u = dg.uniform(sd + 2, B * Nc * H1 * W1 * 2).reshape(B, Nc, H1, W1, 2)
    c = (u * np.array([9.0, 16.0]) - np.array([4.0, 3.0])).astype(F32)
    g = dg.normal(sd + 3, B * Nc * rr * H1 * W1).reshape(B, Nc, rr, H1, W1).astype(F32)
    r1, r2, _ = oracle.alt_corr_backward(f1, f2, c, g, r)
    m1, m2, _ = oracle.alt_corr_backward(np.abs(f1), np.abs(f2), c, np.abs(g), r)
    n1 = sum(_counts(c[:, k], r, H2, W2)[0] for k in range(Nc))[..., None]
    n2 = sum(_counts(c[:, k], r, H2, W2)[1] for k in range(Nc))[..., None]
    assert (n1 == 0).any() and (n2 == 0).any()      # queries off the map, cells never reached
    n1, n2 = n1 + 2, n2 + 2                         # the accumulate's own add, as the block's + 2
    t1, t2, tc, tg = _t(f1), _t(f2), _t(c), _t(g)
    n1e, n2e = f1.size, f2.size

    def run(fill):
        b1 = torch.full((n1e + GUARD,), fill, dtype=torch.float32, device=DEV)
        b2 = torch.full((n2e + GUARD,), fill, dtype=torch.float32, device=DEV)
        b1[n1e:] = SENT
        b2[n2e:] = SENT
        st = lib.dxr_alt_corr_backward(t1.data_ptr(), t2.data_ptr(), tc.data_ptr(), tg.data_ptr(),
                                       b1.data_ptr(), b2.data_ptr(), B, H1, W1, H2, W2, C, Nc,
                                       r | nat.DXR_ALT_BWD_ACCUMULATE, nat.stream_of(b1))
        nat.check(st, "flagged dxr_alt_corr_backward")
        torch.cuda.synchronize()
        assert (b1[n1e:] == SENT).all() and (b2[n2e:] == SENT).all(), "a guard float changed"
        return (b1[:n1e].cpu().numpy().reshape(f1.shape).astype(np.float64),
                b2[:n2e].cpu().numpy().reshape(f2.shape).astype(np.float64))

    zero = run(0.0)
    check("capi zero-filled", zero, (r1, r2), (m1, m2), (n1, n2))
    assert (m1 == 0).any() and (m2 == 0).any()
    pre = run(SENT)
    # an untouched element keeps the sentinel exactly
    assert (pre[0][m1 == 0] == SENT).all() and (pre[1][m2 == 0] == SENT).all()
    # adding into 1.5 rounds each of the element's adds at up to 2^-24 (1.5 + M)
    for name, p, z, m, cnt in zip(("fmap1_grad", "fmap2_grad"), pre, zero, (m1, m2), (n1, n2)):
        assert (np.abs(p - SENT - z) <= 2 * 4.0 * cnt * U * m + cnt * U * (SENT + m)).all(), name
