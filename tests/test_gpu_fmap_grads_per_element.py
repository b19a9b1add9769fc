"""GPU: the fused fmap-gradient GEMMs (``dxr_fmap_grads``,
``dxr_fmap_grads_bounded``) and training through ``CorrBlock``, element by
element against float64.

Every output element of both forms is held to the bound of its arithmetic
(tests/fmap_grads_oracle.py derives both from the stated contract; nothing in
them is measured), on today's N(0, 1) pyramids and on ``wide`` data: fmaps over
17 binades per channel with an outlier pixel and zero channels, gradient rows
that are sparse per query, span 25 binades across queries and are all zero at
every 11th query.  tests/test_fmap_grads_bound_cpu.py shows on the host what
that buys: an arithmetic that reads float16 subnormal operand parts as zero,
drops a low part or a product, or lets a pooled level reach the floor-mode
remainder, exceeds these bounds on the ``wide`` cases, and the first of them is
invisible on the N(0, 1) ones.

Each test prints the largest fraction of its bound any element uses.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import datagen as dg
import fmap_grads_oracle as fo
import oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
IDS = ["x".join(map(str, s)) for s in fo.SHAPES]

# K chunks (dF1, dF2) of each shape under set_kernel's rule: both GEMMs unsplit, split, and mixed
CHUNKS = {fo.SHAPES[0]: (1, 1), fo.SHAPES[1]: (4, 2), fo.SHAPES[2]: (9, 7),
          fo.SHAPES[3]: (4, 3), fo.SHAPES[4]: (9, 8)}


@pytest.fixture(scope="module")
def dx():
    import dexiraft_amd
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    dexiraft_amd.load_native()
    return dexiraft_amd


def _nat():
    from dexiraft_amd import _native
    return _native


def _t(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.array(a)).to(DEV)       # a copy: the cases' arrays are read-only


_DEVICE: dict = {}


def _device(c):
    """(gradient pyramid, fmap1, fmap2) of a case on the device (zero padding)."""
    if c.key not in _DEVICE:
        nat = _nat()
        lib = nat.load()
        gp = torch.zeros(lib.dxr_pyramid_numel(c.B, c.H, c.W, c.L), dtype=torch.float32, device=DEV)
        for lvl, g in enumerate(c.G):
            t = _t(g)
            nat.check(lib.dxr_pyramid_pack(t.data_ptr(), c.B, c.H, c.W, c.L, lvl, gp.data_ptr(),
                                           nat.DXR_F32, nat.stream_of(gp)), "pack")
        torch.cuda.synchronize()
        _DEVICE[c.key] = (gp, _t(c.f1), _t(c.f2))
    return _DEVICE[c.key]


def _six(c, want=(True, True)):
    nat = _nat()
    lib = nat.load()
    gp, f1, f2 = _device(c)
    wsb = lib.dxr_fmap_grads_workspace_bytes(c.B, c.D, c.H, c.W, c.L)
    assert wsb > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    df1 = torch.full_like(f1, float("nan")) if want[0] else None
    df2 = torch.full_like(f2, float("nan")) if want[1] else None
    nat.check(lib.dxr_fmap_grads(gp.data_ptr(), nat.DXR_F32, f1.data_ptr(), f2.data_ptr(), c.B, c.D,
                                 c.H, c.W, c.L, float(c.div), nat.ptr(df1), nat.ptr(df2),
                                 ws.data_ptr(), wsb, nat.stream_of(f1)), "dxr_fmap_grads")
    torch.cuda.synchronize()
    return df1, df2


def _slots(top: float, n: int = 7) -> torch.Tensor:
    """n bound slots whose largest is ``top`` (the rest smaller)."""
    return torch.tensor([np.float32(top) * 0.5 ** k for k in range(n)][::-1], dtype=torch.float32,
                        device=DEV)


def _pair(c, slots, want=(True, True)):
    nat = _nat()
    lib = nat.load()
    gp, f1, f2 = _device(c)
    wsb = lib.dxr_fmap_grads_bounded_workspace_bytes(c.B, c.D, c.H, c.W, c.L)
    assert wsb > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    df1 = torch.full_like(f1, float("nan")) if want[0] else None
    df2 = torch.full_like(f2, float("nan")) if want[1] else None
    nat.check(lib.dxr_fmap_grads_bounded(gp.data_ptr(), nat.DXR_F32, f1.data_ptr(), f2.data_ptr(),
                                         c.B, c.D, c.H, c.W, c.L, float(c.div), slots.data_ptr(),
                                         slots.numel(), nat.ptr(df1), nat.ptr(df2), ws.data_ptr(),
                                         wsb, nat.stream_of(f1)), "dxr_fmap_grads_bounded")
    torch.cuda.synchronize()
    return df1, df2


def _check(tag, c, got, slot_max=None, terms=None, extra=0.0):
    """Both outputs per element: finite, |got - ref| <= the form's bound (the
    f16-pair form's for a ``slot_max``, else the six-product form's) + ``extra``
    x A, and exactly zero where no non-zero product exists."""
    terms = fo.reference(c) if terms is None else terms
    worst = []
    for name, g, f, kt in (("df1", got[0], c.f2, True), ("df2", got[1], c.f1, False)):
        t = terms[name]
        S = fo.k_chunks(c.B, c.D, c.H, c.W, kt)
        g = g.cpu().numpy().astype(np.float64)
        assert np.isfinite(g).all(), (tag, name)
        bound = fo.bound_six(t, c.L, S) if slot_max is None else \
            fo.bound_pair(t, f, slot_max, c.div, c.L, S)
        bound = bound + extra * t["A"]
        err = np.abs(g - t["ref"])
        use = fo.fraction(err, bound)
        i = np.unravel_index(int(np.argmax(np.where(bound > 0, err / bound, 0))), err.shape)
        print(f"{tag} {name}: max err / bound {use:.3f} at {i}: got {g[i]:.9e} ref {t['ref'][i]:.9e} "
              f"A {t['A'][i]:.3e} n {int(t['n'][i])}; max err / max|ref| "
              f"{err.max() / max(np.abs(t['ref']).max(), 1e-300):.3e}")
        worst.append(use)
        zero = t["A"] == 0
        assert zero.any() or c.key[6] == "uniform", (tag, name)
        assert (g[zero] == 0).all(), f"{tag} {name}: an element with no non-zero product is not 0"
        assert use <= 1.0, (tag, name, use)
    return worst


# --------------------------------------------------------------------------- split rule
def test_cases_cover_split_and_unsplit_k(dx):
    """set_kernel's rule (restated in fmap_grads_oracle.k_chunks): which shapes
    split K in which GEMM.  Both kernels run unsplit and split."""
    for shape in fo.SHAPES:
        assert (fo.k_chunks(*shape[:4], True), fo.k_chunks(*shape[:4], False)) == CHUNKS[shape]
    for side in range(2):
        assert {CHUNKS[s][side] == 1 for s in fo.SHAPES} == {True, False}
    # the workspace the library asks for is the restated rule's, so the rule is the library's
    lib = _nat().load()
    for (B, D, H, W, L), (s1, s2) in CHUNKS.items():
        qt, tiles = -(-(H * W) // 128), -(-H // 8) * -(-W // 16)
        a256 = lambda x: -(-x // 256) * 256  # noqa: E731
        need = max(a256((2 + B * D) * 4) + a256(B * 2 * kbt * 8 * D * 32) +
                   (a256((S - 1) * B * D * H * W * 4) if S > 1 else 0)
                   for kbt, S in ((tiles, s1), (qt, s2)))
        assert lib.dxr_fmap_grads_bounded_workspace_bytes(B, D, H, W, L) == need


# --------------------------------------------------------------------------- per element
@pytest.mark.parametrize("form", ["six", "pair_tight", "pair_loose"])
@pytest.mark.parametrize("kind", ["uniform", "wide"])
@pytest.mark.parametrize("shape", fo.SHAPES, ids=IDS)
def test_fmap_grads_per_element(dx, shape, kind, form):
    """Both forms, both outputs, against float64 and the bound of the form; the
    bounded form with a tight slot bound (max|G|) and one loose by 3000x (the
    dV scale follows the slots)."""
    c = fo.shape_case(shape, kind)
    tag = f"{shape} {kind} {form}"
    if form == "six":
        _check(tag, c, _six(c))
    else:
        top = float(np.float32(c.gmax) * np.float32(1.0 if form == "pair_tight" else 3000.0))
        _check(tag, c, _pair(c, _slots(top)), slot_max=top)


# --------------------------------------------------------------------------- scale edges
def _edge():
    return fo.shape_case(fo.EDGE_SHAPE, "wide")


@pytest.mark.parametrize("g_exp", [-100, 100])
def test_bounded_gradient_scale_edges(dx, g_exp):
    """G x 2^-100 (the small queries' gradients are float32 subnormals) and
    x 2^100, the slots scaled alike: every term of the bound scales with them."""
    c = fo.rescaled(_edge(), g_exp=g_exp)
    _check(f"G x 2^{g_exp}", c, _pair(c, _slots(c.gmax)), slot_max=c.gmax)


def test_bounded_tiny_fmaps(dx):
    """fmaps x 2^-120: channel maxima down to 2^-128 (the scale clamp at 125),
    float32-subnormal fmap values, outputs in and near the float32 subnormal
    range, where the bound's absolute steps take over."""
    c = fo.rescaled(_edge(), f_exp=-120)
    assert (fo.scale_for(np.abs(c.f2).reshape(c.B, c.D, -1).max(axis=2)) == 125).any()
    ref = fo.reference(c)["df1"]["ref"]
    assert ((np.abs(ref) < 2.0 ** -126) & (ref != 0)).any()
    _check("fmaps x 2^-120", c, _pair(c, _slots(c.gmax)), slot_max=c.gmax)


def test_bounded_zero_gradient(dx):
    """G all zero, every slot zero: exactly zero outputs."""
    e = _edge()
    c = fo.rescaled(fo.rescaled(e, zero_pair=0), zero_pair=1)
    assert c.gmax == 0
    g1, g2 = _pair(c, torch.zeros(5, dtype=torch.float32, device=DEV))
    assert not g1.any() and not g2.any()


def test_bounded_zero_pair_beside_a_large_one(dx):
    """Pair 0's G all zero, pair 1's x 2^20: pair 0's gradients are exactly zero
    (checked by A == 0), pair 1's within the bound."""
    c = fo.rescaled(_edge(), g_exp=20, zero_pair=0)
    g1, g2 = _pair(c, _slots(c.gmax))
    assert not g1[0].any() and not g2[0].any()
    _check("zero pair", c, (g1, g2), slot_max=c.gmax)


def test_bounded_inf_slot_takes_the_six_product_path(dx):
    """One +inf slot among finite ones: the bound is not finite, the whole call
    runs the six-product arithmetic: dxr_fmap_grads' outputs bit for bit."""
    c = _edge()
    sl = _slots(c.gmax)
    sl[2] = float("inf")
    g1, g2 = _pair(c, sl)
    u1, u2 = _six(c)
    assert torch.isfinite(u1).all() and torch.isfinite(u2).all()
    assert torch.equal(g1, u1) and torch.equal(g2, u2)
    p1, _ = _pair(c, _slots(c.gmax))
    assert not torch.equal(p1, u1)           # and the f16-pair form is another arithmetic


@pytest.mark.parametrize("form", ["six", "pair"])
def test_one_sided_calls_equal_the_two_sided_call(dx, form):
    c = _edge()
    run = _six if form == "six" else (lambda c, want=(True, True): _pair(c, _slots(c.gmax), want))
    a1, a2 = run(c)
    b1, n2 = run(c, want=(True, False))
    n1, b2 = run(c, want=(False, True))
    assert n1 is None and n2 is None
    assert torch.equal(a1, b1) and torch.equal(a2, b2)


# --------------------------------------------------------------------------- whole block
def _block_weights(seed, B, K, H, W, k, bf16_exact):
    """Loss weights of lookup k, [B, K, H, W] float32: 1, 2, 5, 16 or about 100
    non-zero channels per pixel, per-pixel scale 2^-(q % 25), every 11th pixel
    (an invalid one) zero; lookup 3's all zero."""
    BN = B * H * W
    q = np.arange(BN)
    cnt = np.minimum(np.asarray(fo.SPARSITY)[(q + k) % len(fo.SPARSITY)], K)
    u = dg.uniform(seed + 2 * k, BN * K).reshape(BN, K)
    mask = u <= np.sort(u, axis=1)[q, cnt - 1][:, None]
    w = dg.normal(seed + 2 * k + 1, BN * K).reshape(BN, K) * mask * np.exp2(-(q % 25.0))[:, None]
    w[q % 11 == 0] = 0.0
    if k == 3:
        w[:] = 0.0
    w = np.ascontiguousarray(w.reshape(B, H, W, K).transpose(0, 3, 1, 2)).astype(np.float32)
    if bf16_exact:      # values a bfloat16 holds: the cast of the 16-bit lookup's gradient is exact
        w = (w.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    return w


BLOCKS = {
    "23x37_L3_r3": dict(B=1, D=64, H=23, W=37, L=3, r=3),
    "18x21_L4_r4": dict(B=2, D=64, H=18, W=21, L=4, r=4),
    "23x37_L3_r3_channels_last_fmaps": dict(B=1, D=64, H=23, W=37, L=3, r=3, cl_fmaps=True),
    "18x21_L4_r4_bf16_channels_last_lookups": dict(B=2, D=64, H=18, W=21, L=4, r=4, out16=True),
}


@pytest.mark.parametrize("name", list(BLOCKS))
def test_corr_block_backward_per_element(dx, name):
    """Training through CorrBlock, five lookups (lookup backwards flushed two,
    two and one at the build), loss sum_k <cb(c_k), w_k> with sparse,
    heavy-tailed w_k.  Reference: oracle.corr_lookup_backward summed over the
    lookups, then oracle.corr_pyramid_backward, float64.  Bound: the f16-pair
    GEMM bound on the lookup backward's magnitude pyramid M (the same oracle on
    |w_k|), plus 2^-20 of the A computed from M: the per-cell rule of
    test_lookup_backward_matches_oracle_per_cell (zero base), pushed through
    the linear fold and GEMM.  The dV scale is that of the slots' documented
    ceiling 9 sum_k max|w_k| (1 + 1e-6).  Invalid pixels' dfmap1 columns are
    exactly zero."""
    p = BLOCKS[name]
    B, D, H, W, L, r = (p[k] for k in "BDHWLr")
    out16, cl = p.get("out16", False), p.get("cl_fmaps", False)
    seed = 5200 + 50 * list(BLOCKS).index(name)
    K = L * (2 * r + 1) ** 2
    wide = fo.case(seed, B, D, H, W, 1, "wide")           # its fmaps only
    f1, f2 = wide.f1, wide.f2
    cs = [dg.coords(seed + 10 + k, B, H, W, "normal", 3.0) for k in range(5)]
    ws = [_block_weights(seed + 20, B, K, H, W, k, out16) for k in range(5)]
    assert not ws[3].any()

    shapes = fo.level_shapes(H, W, L)
    ref = [np.zeros((B * H * W,) + s) for s in shapes]
    mag = [np.zeros_like(a) for a in ref]
    for c, w in zip(cs, ws):
        for a, x in zip(ref, oracle.corr_lookup_backward(shapes, c, r, w)):
            a += x
        for a, x in zip(mag, oracle.corr_lookup_backward(shapes, c, r, np.abs(w))):
            a += x
    assert all((m > 0).any() for m in mag)
    terms = fo.gemm_terms(f1, f2, ref, mag)
    ceiling = 9.0 * sum(float(np.abs(w).max()) for w in ws) * (1 + 1e-6)

    a1, a2 = _t(f1), _t(f2)
    if cl:
        a1, a2 = (a.contiguous(memory_format=torch.channels_last) for a in (a1, a2))
    a1.requires_grad_(True)
    a2.requires_grad_(True)
    cb = dx.CorrBlock(a1, a2, num_levels=L, radius=r)
    kw = dict(out_dtype=torch.bfloat16, memory_format=torch.channels_last) if out16 else {}
    loss = sum((cb(_t(c), **kw) * _t(w)).sum() for c, w in zip(cs, ws))
    loss.backward()
    torch.cuda.synchronize()

    class _C:       # what _check reads of a case
        key = (0, 0, 0, 0, 0, 0, "wide")
    _C.B, _C.D, _C.H, _C.W, _C.L, _C.f1, _C.f2, _C.div = B, D, H, W, L, f1, f2, wide.div
    _check(name, _C, (a1.grad, a2.grad), slot_max=ceiling, terms=terms, extra=2.0 ** -20)
    dead = (np.arange(B * H * W) % 11 == 0).reshape(B, H, W)
    g1 = a1.grad.cpu().numpy()
    assert (g1.transpose(0, 2, 3, 1)[dead] == 0).all()
    assert (g1.transpose(0, 2, 3, 1)[~dead] != 0).any()
