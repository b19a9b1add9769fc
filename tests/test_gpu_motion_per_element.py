"""The lookup fused with convc1 (``CorrBlock.lookup_conv1x1`` ->
``corr_lookup_conv1x1_h2_kernel``), every output element against float64 with
the bounds derived in tests/motion_oracle.py, in both workgroup forms.

The samples come from hand-made pyramids (reference-layout levels filled on the
device from a seeded generator, packed by ``dxr_pyramid_pack`` into the buffer
of a real block), so their magnitudes are controlled.  The operand x of every
reference is the block's own unfused lookup ``cb(coords)``, which has its own
per-output tests and is not under test here.

Forms: (B, H, W) = (2, 16, 17) is 9 workgroups per item, the last ragged, 18 in
all: the 1024-thread KSPLIT = 2 form; (3, 53, 53) is 88 per item (2809 % 32 =
25), 264 in all: the 512-thread form.  (2, 9, 13), 4 workgroups per item, runs
the 1024-thread form with one and two levels only: its fourth level is 1 x 1,
where the lookup's samples are NaN as the reference's are (2 c / (W - 1) - 1),
so no bound on finite outputs can be asked there.

Largest fraction of a bound used on an MI355X: see DESIGN.md and the log under
profiles/r25.
"""
from __future__ import annotations

from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import datagen as dg
import motion_oracle as mo

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
D = 32
FORMS = {"t1024": (2, 16, 17), "t512": (3, 53, 53), "t1024s": (2, 9, 13)}
MAIN = ["t1024", "t512"]
# every (levels, radius) on the main forms; the small one where every level is at least 2 x 2
CASES = [(f, L, r) for f in FORMS for L, r in mo.CONFIGS
         if min(FORMS[f][1:]) >> (L - 1) >= 2 and (f in MAIN or L <= 2)]
COUTS = (32, 96, 288)
# (item, query) with integer coordinates on a level-0 cell of 65519, where the reference's float32
# 2 c / (size - 1) - 1 and back returns the integer exactly (row 0; 2 x / (W - 1) exact)
TOPS = {"t1024": (0, 12), "t512": (0, 26), "t1024s": (0, 12)}
BIG = (1, 50)     # (item, query): integer coordinates; the 1e6 cell of the one-workgroup fallback
ZERO_MOD = 37     # queries q % 37 == 5 sample nothing but zeros


@pytest.fixture(scope="module")
def dx():
    import dexiraft_amd
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    dexiraft_amd.load_native()
    return dexiraft_amd


def _t(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _sizes(H, W, L=4):
    return [(H >> lvl, W >> lvl) for lvl in range(L)]


# --------------------------------------------------------------------------- inputs
@lru_cache(maxsize=None)
def _levels(form: str, kind: str) -> tuple:
    """Four reference-layout levels [B*N, 1, h, w] float32 on the device.
    ``unit``: N(0, 1).  ``wide``: N(0, 1) 2^e, e in [-30, 10]; a query's whole
    level zero with probability 0.1 (exact-zero samples); the first 8 queries of
    every workgroup a further 2^-20; queries q % 37 == 5 zero on every level; one
    level-0 cell of exactly 65519 under the form's query of TOPS."""
    B, H, W = FORMS[form]
    N = H * W
    g = torch.Generator(device=DEV).manual_seed(2500 + 10 * list(FORMS).index(form) + (kind == "wide"))
    q = (torch.arange(B * N, device=DEV) % N).view(-1, 1, 1, 1)
    levels = []
    for h, w in _sizes(H, W):
        v = torch.randn((B * N, 1, h, w), generator=g, device=DEV)
        if kind == "wide":
            v = torch.ldexp(v, torch.randint(-30, 11, v.shape, generator=g, device=DEV))
            v = v * (torch.rand((B * N, 1, 1, 1), generator=g, device=DEV) >= 0.1)
            v = v * torch.where(q % mo.QB < 8, 2.0 ** -20, 1.0) * (q % ZERO_MOD != 5)
        levels.append(v.float().contiguous())
    if kind == "wide":
        b, t = TOPS[form]
        levels[0][b * N + t, 0, t // W, t % W] = mo.X_TOP
    return tuple(levels)


@lru_cache(maxsize=None)
def _coords(form: str) -> torch.Tensor:
    B, H, W = FORMS[form]
    c = dg.coords(2590 + list(FORMS).index(form), B, H, W, "normal", 3.0)
    for b, q in (TOPS[form], BIG):
        c[b, :, q // W, q % W] = (q % W, q // W)
    return _t(c)


def _hand_block(form: str, L: int, r: int, levels):
    """A real float32 block of the form's geometry whose pyramid buffer is replaced
    by a zero-filled one holding ``levels`` (tests/test_gpu_pyr16.py
    ``_widened_f32_block``)."""
    import dexiraft_amd
    from dexiraft_amd import _native as nat
    B, H, W = FORMS[form]
    cb = dexiraft_amd.CorrBlock(_t(dg.fmap(2580, B, D, H, W, "fnet")), _t(dg.fmap(2581, B, D, H, W, "fnet")),
                                num_levels=L, radius=r)
    assert cb._pyr_dt == nat.DXR_F32 and cb._buf.dtype == torch.float32
    lib = nat.load()
    buf = torch.zeros(cb._buf.numel(), dtype=torch.float32, device=DEV)
    for lvl, lev in enumerate(levels):
        assert lev.shape == (B * H * W, 1, *_sizes(H, W)[lvl]) and lev.is_contiguous()
        assert lib.dxr_pyramid_pack(lev.data_ptr(), B, H, W, L, lvl, buf.data_ptr(), nat.DXR_F32,
                                    nat.stream_of(buf)) == nat.DXR_OK
    cb._buf, cb._ref_pyramid = buf, None
    return cb


def _flat(t: torch.Tensor) -> np.ndarray:
    """[B, C, H, W] (any memory format) -> numpy [C, B*N], queries item by item."""
    a = t.cpu().numpy()
    return np.ascontiguousarray(a.reshape(a.shape[0], a.shape[1], -1).transpose(1, 0, 2)).reshape(a.shape[1], -1)


def _wrap(form: str, cb) -> SimpleNamespace:
    B, H, W = FORMS[form]
    c = _coords(form)
    x = _flat(cb(c))
    return SimpleNamespace(cb=cb, c=c, x=x, B=B, N=H * W, cin=x.shape[0], ksplit=mo.ksplit_of(B, H * W))


@lru_cache(maxsize=2)
def _case(form: str, L: int, r: int, kind: str) -> SimpleNamespace:
    cs = _wrap(form, _hand_block(form, L, r, _levels(form, kind)[:L]))
    assert cs.cin == mo.cin_of(L, r) and np.isfinite(cs.x).all()
    return cs


@lru_cache(maxsize=None)
def _weights(kind: str, cin: int):
    return (mo.unit_weights if kind == "unit" else mo.wide_weights)(2600 + cin, max(COUTS), cin)


@lru_cache(maxsize=2)
def _terms(form: str, L: int, r: int, kind: str) -> dict:
    return mo.terms(_weights(kind, mo.cin_of(L, r))[0], _case(form, L, r, kind).x)


def _emulated(cs, w, bias) -> np.ndarray:
    return np.concatenate([mo.emulate(w, cs.x[:, i:i + cs.N], bias, cs.ksplit)[0]
                           for i in range(0, cs.B * cs.N, cs.N)], axis=1)


# --------------------------------------------------------------------------- 1. the bound
@pytest.mark.parametrize("kind", ["unit", "wide"])
@pytest.mark.parametrize("form,L,r", CASES)
def test_every_element_within_the_pair_bound(dx, form, L, r, kind):
    cs = _case(form, L, r, kind)
    w, bias = _weights(kind, cs.cin)
    t_all = _terms(form, L, r, kind)
    assert (cs.ksplit == 2) == (form != "t512")
    if kind == "wide":
        assert np.abs(cs.x).max() < mo.F16_LIMIT
        assert (cs.x[:, TOPS[form][0] * cs.N + TOPS[form][1]] == np.float32(mo.X_TOP)).sum() == 1
        # a tenth of the levels are zero; so are the taps that fall off the map
        assert 0.1 < (cs.x == 0).mean() < 0.9 and (t_all["M0"] == 0).any()
        m = np.abs(cs.x[cs.x != 0])
        assert (m < 2.0 ** -25).mean() > 0.05 and (m >= mo.F16_MIN_NORMAL).mean() > 0.1
    for cout in COUTS:
        t = mo.rows(t_all, cout)
        wd, bd, bnp = _t(w[:cout]), _t(bias[:cout]), bias[:cout]
        for b, mf in ((bd, None), (None, None), (bd, torch.channels_last)):
            out = cs.cb.lookup_conv1x1(cs.c, wd, b, relu=False, memory_format=mf)
            assert out.dtype == torch.float32 and out.shape[1] == cout
            assert out.is_contiguous(memory_format=mf or torch.contiguous_format)
            got = _flat(out)
            bb = None if b is None else bnp
            f = mo.fraction(got, mo.reference(t, bb), mo.bound_pair(t, bb, cs.ksplit))
            print(f"{form} L{L} r{r} {kind} cout {cout} bias {b is not None} "
                  f"{'nhwc' if mf else 'nchw'}: {f:.4f} of the bound")
            assert np.isfinite(got).all()
            assert f <= 1.0
            zero = t["M0"] == 0
            want = np.broadcast_to(np.zeros(cout, np.float32) if b is None else bnp, got.T.shape).T
            assert np.array_equal(got[zero], want[zero])
        if cout == COUTS[0] or cs.B * cs.N < 1000:    # what the host emulation of the same arithmetic uses
            emu = _emulated(cs, w[:cout], bnp)
            fe = mo.fraction(emu, mo.reference(t, bnp), mo.bound_pair(t, bnp, cs.ksplit))
            same = (emu == _flat(cs.cb.lookup_conv1x1(cs.c, wd, bd, relu=False))).mean()
            print(f"{form} L{L} r{r} {kind} cout {cout}: the emulation uses {fe:.4f}; "
                  f"{same:.4f} of the GPU's elements equal it bit for bit")


# --------------------------------------------------------------------------- 2. one-hot weights
@pytest.mark.parametrize("form", MAIN)
def test_one_hot_weights_return_the_lookups_samples(dx, form):
    """cout = 352 >= cin = 324: row o picks channel o (1.0 = hi exactly, lo = 0), so
    the output is hi + lo / 2048 of the lookup's sample: within e(|x|) of it, in the
    lookup's channel order; rows beyond cin are zero.  11 output blocks: the second
    pass over the rows has 3 of 8 waves (6 of 16) active."""
    cs = _case(form, 4, 4, "wide")
    cout = 352
    w = np.zeros((cout, cs.cin), dtype=np.float32)
    w[np.arange(cs.cin), np.arange(cs.cin)] = 1.0
    got = _flat(cs.cb.lookup_conv1x1(cs.c, _t(w), None, relu=False))
    assert got.shape == (cout, cs.B * cs.N) and np.isfinite(got).all()
    assert (got[cs.cin:] == 0).all()
    err = np.abs(got[:cs.cin].astype(np.float64) - cs.x)
    tol = mo.e_of(cs.x)
    with np.errstate(divide="ignore", invalid="ignore"):
        use = np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.0))
    print(f"{form} one-hot: {use.max():.4f} of e(|x|); {(got[:cs.cin] == cs.x).mean():.4f} of the "
          f"samples returned bit for bit")
    assert (err <= tol).all()
    top = cs.x == np.float32(mo.X_TOP)       # 65504 + 30720 / 2048: returned exactly
    assert top.any() and (got[:cs.cin][top] == np.float32(mo.X_TOP)).all()


# --------------------------------------------------------------------------- 3. ReLU, determinism
@pytest.mark.parametrize("form", MAIN)
def test_relu_is_relu_of_the_linear_output_and_calls_repeat(dx, form):
    cs = _case(form, 4, 4, "wide")
    w, bias = _weights("wide", cs.cin)
    wd, bd = _t(w), _t(bias)
    lin = cs.cb.lookup_conv1x1(cs.c, wd, bd, relu=False)
    act = cs.cb.lookup_conv1x1(cs.c, wd, bd, relu=True)
    assert torch.isfinite(lin).all() and (lin < 0).any() and (lin > 0).any()
    assert torch.equal(act.view(torch.int32), torch.where(lin < 0, 0.0, lin).view(torch.int32))
    assert torch.equal(act, torch.relu(lin))
    for relu, first in ((False, lin), (True, act)):
        again = cs.cb.lookup_conv1x1(cs.c, wd, bd, relu=relu)
        assert torch.equal(again.view(torch.int32), first.view(torch.int32))


# --------------------------------------------------------------------------- 4. fallback, whole grid
@pytest.mark.parametrize("form", MAIN)
def test_fallback_of_every_workgroup(dx, form):
    """One weight of 1e5 (inf in float16) on a channel with a non-zero sample in
    every workgroup: every workgroup's pair sums are non-finite and it repeats its
    GEMM on the three-way bf16 split."""
    cs = _case(form, 4, 4, "wide")
    w, bias = _weights("wide", cs.cin)
    w, c = mo.with_overflowing_weight(w, cs.x, cs.N)
    for a in (w, cs.x):
        assert np.abs(a[a != 0]).min() >= 2.0 ** -100
    t = mo.terms(w, cs.x)
    got = _flat(cs.cb.lookup_conv1x1(cs.c, _t(w), _t(bias), relu=False))
    f = mo.fraction(got, mo.reference(t, bias), mo.bound_six(t, bias, cs.ksplit))
    print(f"{form} fallback of every workgroup (1e5 on channel {c}): {f:.4f} of the bound")
    assert np.isfinite(got).all()
    assert f <= 1.0


# --------------------------------------------------------------------------- 5. fallback, one workgroup
@pytest.mark.parametrize("zero_weights", [False, True], ids=["inf", "inf_times_0"])
@pytest.mark.parametrize("form", MAIN)
def test_fallback_of_one_workgroup(dx, form, zero_weights):
    """A level-0 cell of 1e6 under query BIG alone: its sample is inf in float16,
    so that query's workgroup (32 consecutive queries of its item) falls back and
    the others do not.  ``inf_times_0``: every weight on that channel is zero, the
    pair path's inf * 0 is NaN, and the result has to be finite and right."""
    B, H, W = FORMS[form]
    N, (b, q) = H * W, BIG
    levels = list(_levels(form, "wide"))
    levels[0] = levels[0].clone()
    levels[0][b * N + q, 0, q // W, q % W] = 1e6
    cs = _wrap(form, _hand_block(form, 4, 4, levels))
    over = np.abs(cs.x) >= mo.F16_LIMIT
    chans = np.flatnonzero(over.any(axis=1))
    assert len(chans) >= 1 and over.any(axis=0).sum() == 1 and over[:, b * N + q].any()
    cout = 96
    w, bias = (a[:cout].copy() for a in _weights("wide", cs.cin))
    if zero_weights:
        w[:, chans] = 0.0
    else:
        assert (w[:, chans] != 0).all()
    fell = np.zeros(B * N, dtype=bool)          # from the geometry alone
    fell[b * N + q // mo.QB * mo.QB: b * N + min((q // mo.QB + 1) * mo.QB, N)] = True
    assert fell.sum() == mo.QB
    t = mo.terms(w, cs.x)
    bound = np.where(fell[None, :], mo.bound_six(t, bias, cs.ksplit), mo.bound_pair(t, bias, cs.ksplit))
    got = _flat(cs.cb.lookup_conv1x1(cs.c, _t(w), _t(bias), relu=False))
    ref = mo.reference(t, bias)
    f_in = mo.fraction(got[:, fell], ref[:, fell], bound[:, fell])
    f_out = mo.fraction(got[:, ~fell], ref[:, ~fell], bound[:, ~fell])
    print(f"{form} one workgroup falls back ({'zero' if zero_weights else 'non-zero'} weights on "
          f"channels {list(chans)}): {f_in:.4f} of the fallback bound inside, {f_out:.4f} of the pair "
          f"bound outside")
    assert np.isfinite(got).all()
    assert f_in <= 1.0 and f_out <= 1.0


# --------------------------------------------------------------------------- 6. 16-bit pyramids
@pytest.mark.parametrize("pyr", ["f16", "bf16"])
def test_16_bit_pyramids_in_the_512_thread_form(dx, pyr):
    """Built blocks whose pyramid is float16 / bfloat16: only the samples differ, the
    contraction and its bound are the same.  Two calls are bit-identical."""
    form = "t512"
    B, H, W = FORMS[form]
    f1, f2 = _t(dg.fmap(2680, B, D, H, W, "fnet")), _t(dg.fmap(2681, B, D, H, W, "fnet"))
    if pyr == "f16":
        cb = dx.CorrBlock(f1, f2, pyramid_dtype=torch.float16)
        assert cb._buf.dtype == torch.float16
    else:
        cb = dx.CorrBlock(f1.bfloat16(), f2.bfloat16())
        assert cb._buf.dtype == torch.bfloat16
    cs = _wrap(form, cb)
    assert cs.ksplit == 1 and (cs.x != 0).any()
    cout = 96
    w, bias = (a[:cout] for a in _weights("unit", cs.cin))
    t = mo.terms(w, cs.x)
    out = cs.cb.lookup_conv1x1(cs.c, _t(w), _t(bias), relu=False)
    got = _flat(out)
    f = mo.fraction(got, mo.reference(t, bias), mo.bound_pair(t, bias, cs.ksplit))
    print(f"{form} {pyr} pyramid, unit weights: {f:.4f} of the bound")
    assert np.isfinite(got).all()
    assert f <= 1.0
    again = cs.cb.lookup_conv1x1(cs.c, _t(w), _t(bias), relu=False)
    assert torch.equal(again.view(torch.int32), out.view(torch.int32))
