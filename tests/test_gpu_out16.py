"""GPU: float16 / bfloat16 lookup outputs (``out_dtype`` of CorrBlock.__call__ and
lookup_conv1x1; DXR_OUT_F16 / DXR_OUT_BF16 at the C-ABI).

The contract is "autocast's cast, fused into the store": the 16-bit result is the
float32 result's ``.to(dtype)`` bit for bit (round to nearest even, float16
overflow to +-inf, float16 subnormals kept), NaNs in the same positions.  So the
reference everywhere is the float32 call of the same block followed by torch's
cast, and there is no tolerance.

Shapes follow the store scheme (corr_lookup_qm_kernel: lanes 2i, 2i + 1 hold
queries q, q + 1 of one channel row and write one 32-bit word where it is 4-byte
aligned, single 16-bit elements elsewhere):

  a  B=2 D=32  9x13   N = 117 odd: every second channel row is unaligned (single
                      stores), an odd tail query; batch offset; write-through stores
  b  B=1 D=32  10x13  N = 130: even, not a multiple of 16: packed words and a
                      partial workgroup
  c  B=1 D=64  16x24  N = 384, a multiple of 32: the non-temporal branch
  d  B=3 D=32  48x64  more than 1024 32-query workgroups: the multi-round
                      512-thread shape
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest
import torch

import datagen as dg

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = {"a": (2, 32, 9, 13), "b": (1, 32, 10, 13), "c": (1, 64, 16, 24), "d": (3, 32, 48, 64)}
SEEDS = {"a": 1810, "b": 1820, "c": 1830, "d": 1840}
OUT = {"f16": torch.float16, "bf16": torch.bfloat16}
FMAP = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}

# (case, radius, num_levels): r = 4, 3, 1 on a-c; r = 6 (the R > 4 instantiation,
# 16-query workgroups of 512 threads) on b and on the odd-N case; d at r = 4; two levels
LOOKUPS = ([(c, r, 4) for c in "abc" for r in (4, 3, 1)]
           + [("b", 6, 4), ("a", 6, 4), ("d", 4, 4), ("c", 4, 2)])


@pytest.fixture(scope="module")
def dx():
    import dexiraft_amd
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    dexiraft_amd.load_native()
    return dexiraft_amd


def _t(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@lru_cache(maxsize=None)
def _fmaps(case: str, fdt: str, scale: float = 1.0):
    B, D, H, W = CASES[case]
    s = SEEDS[case]
    f1 = _t(dg.fmap(s, B, D, H, W, "fnet") * np.float32(scale)).to(FMAP[fdt])
    f2 = _t(dg.fmap(s + 1, B, D, H, W, "fnet") * np.float32(scale)).to(FMAP[fdt])
    return f1, f2


@lru_cache(maxsize=None)
def _block(case: str, fdt: str, r: int = 4, levels: int = 4, scale: float = 1.0):
    """One block per configuration, shared by the tests (never modified)."""
    import dexiraft_amd
    f1, f2 = _fmaps(case, fdt, scale)
    with torch.no_grad():
        return dexiraft_amd.CorrBlock(f1, f2, num_levels=levels, radius=r)


@lru_cache(maxsize=None)
def _coords(case: str, mode: str = "uniform", scale: float = 6.0):
    B, D, H, W = CASES[case]
    return _t(dg.coords(SEEDS[case] + 2, B, H, W, mode, scale))   # uniform 6: windows partly off the map


def _bits(t: torch.Tensor) -> torch.Tensor:
    assert t.dtype in (torch.float16, torch.bfloat16)
    return t.contiguous().view(torch.int16)


def assert_bit_equal(got: torch.Tensor, ref32: torch.Tensor, dt: torch.dtype, what: str = ""):
    """got == ref32.to(dt): the same 16-bit patterns wherever the reference is not
    NaN, NaN in exactly the reference's NaN positions."""
    assert ref32.dtype == torch.float32
    assert got.dtype == dt and got.is_contiguous() and got.shape == ref32.shape, what
    ref = ref32.to(dt)
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaN positions differ"
    gb, rb = _bits(got), _bits(ref)
    bad = (gb != rb) & ~nan
    nbad = int(bad.sum().item())
    if nbad:
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {nbad} of {bad.numel()} elements differ; first at {i}: got "
                             f"{gb[i].item() & 0xffff:#06x}, want {rb[i].item() & 0xffff:#06x} "
                             f"(float32 {ref32[i].item()!r})")


# ------------------------------------------------------------- 1. bit equality
@pytest.mark.parametrize("odt", ["f16", "bf16"])
@pytest.mark.parametrize("fdt", ["f32", "f16"])
@pytest.mark.parametrize("case,r,levels", LOOKUPS)
def test_out16_equals_cast_of_f32_lookup(dx, case, r, levels, fdt, odt):
    cb = _block(case, fdt, r, levels)
    assert cb._buf.dtype == torch.float32
    c = _coords(case)
    ref = cb(c)
    assert ref.dtype == torch.float32
    got = cb(c, out_dtype=OUT[odt])
    assert_bit_equal(got, ref, OUT[odt], f"{case} r{r} L{levels} {fdt}->{odt}")
    assert torch.isfinite(ref).any() and (ref != 0).any()
    # the float32 call is untouched by the 16-bit one
    assert torch.equal(torch.nan_to_num(cb(c)), torch.nan_to_num(ref))


@pytest.mark.parametrize("case,r,levels,odt",
                         [(c, r, L, "bf16") for c, r, L in LOOKUPS] + [("a", 4, 4, "f16"),
                                                                       ("c", 4, 4, "f16")])
def test_out16_from_bf16_pyramid(dx, case, r, levels, odt):
    cb = _block(case, "bf16", r, levels)
    assert cb._buf.dtype == torch.bfloat16
    c = _coords(case)
    assert_bit_equal(cb(c, out_dtype=OUT[odt]), cb(c), OUT[odt], f"{case} r{r} L{levels} bf16->{odt}")


# ------------------------------------------------------------------- 2. range
F16_MIN_NORMAL = 2.0 ** -14
F16_OVERFLOW = 65520.0    # the first float32 magnitude that rounds to float16 inf


@pytest.mark.parametrize("odt", ["f16", "bf16"])
@pytest.mark.parametrize("case", ["a", "c"])
def test_out16_subnormals_kept(dx, case, odt):
    """fmaps x 1e-3: the correlations (x 1e-6) sit on float16's subnormal grid.
    They must come out as torch's cast gives them, not flushed to zero.
    (float64 oracle on these seeds: case a 17,382 of 75,816 outputs float16-subnormal,
    18,954 NaN (level 3 is one row), the rest 0; case c 55,925 of 124,416.)"""
    cb = _block(case, "f32", 4, 4, 1e-3)
    c = _coords(case)
    ref = cb(c)
    a = ref.abs()
    sub = (a >= 2.0 ** -25) & (a < F16_MIN_NORMAL)     # rounds to a non-zero float16 subnormal
    n_sub = int(sub.sum().item())
    print(f"case {case}: {n_sub} of {ref.numel()} outputs are float16-subnormal, "
          f"{int((ref == 0).sum().item())} zero, max |x| {a[~torch.isnan(a)].max().item():.3e}")
    assert n_sub > ref.numel() // 10
    h = ref.to(torch.float16)
    assert int(((h != 0) & (h.abs() < F16_MIN_NORMAL)).sum().item()) > ref.numel() // 10
    assert_bit_equal(cb(c, out_dtype=OUT[odt]), ref, OUT[odt], f"{case} x1e-3 ->{odt}")


@pytest.mark.parametrize("odt", ["f16", "bf16"])
@pytest.mark.parametrize("case", ["a", "c"])
def test_out16_overflow_to_inf(dx, case, odt):
    """fmaps x 300: most correlations (x 9e4) exceed float16's 65504 and become
    +-inf, as in torch's cast; samples with taps off the map stay finite.
    (float64 oracle on these seeds: case a 16,050 of 75,816 outputs >= 65520 and
    1,428 non-zero below 65504; case c 54,087 and 1,943 of 124,416.)"""
    cb = _block(case, "f32", 4, 4, 300.0)
    c = _coords(case)
    ref = cb(c)
    a = ref.abs()
    over = a >= F16_OVERFLOW
    fin = a < 65504.0
    n_over, n_fin = int(over.sum().item()), int((fin & (a > 0)).sum().item())
    print(f"case {case}: {n_over} of {ref.numel()} outputs overflow float16, {n_fin} non-zero finite")
    assert torch.isfinite(ref[~torch.isnan(ref)]).all()      # finite in float32
    assert n_over > ref.numel() // 10 and n_fin > ref.numel() // 100
    if odt == "f16":
        assert int(torch.isinf(ref.to(torch.float16)).sum().item()) == n_over
    assert_bit_equal(cb(c, out_dtype=OUT[odt]), ref, OUT[odt], f"{case} x300 ->{odt}")


# --------------------------------------- 3. non-finite and far coordinates
@pytest.mark.parametrize("odt", ["f16", "bf16"])
@pytest.mark.parametrize("fdt", ["f32", "bf16"])
def test_out16_far_nan_inf_coords(dx, fdt, odt):
    """The coordinate sets of test_gpu_parity's far / NaN / inf test, and the same
    entries dropped into ordinary coordinates."""
    H, W = 20, 24
    f1 = _t(dg.fmap(41, 1, 32, H, W, "fnet")).to(FMAP[fdt])
    f2 = _t(dg.fmap(42, 1, 32, H, W, "fnet")).to(FMAP[fdt])
    cb = dx.CorrBlock(f1, f2)
    far = _t(dg.coords(43, 1, H, W, "far"))
    c2 = far.clone()
    c2[0, 0, 3, 5] = float("nan")
    c3 = far.clone()
    c3[0, 1, 0, 0] = float("inf")
    c4 = _t(dg.coords(44, 1, H, W, "normal", 4.0))
    c4[0, 0, 3, 5] = float("nan")
    c4[0, 1, 0, 0] = float("inf")
    c4[0, 0, 7, 7] = float("-inf")
    c4[0, :, 10, 11] = 1.0e9
    c4[0, :, 19, 23] = far[0, :, 19, 23]
    dt = OUT[odt]
    for name, c in (("far", far), ("far+nan", c2), ("far+inf", c3), ("normal+nan/inf/far", c4)):
        ref = cb(c)
        got = cb(c, out_dtype=dt)
        assert_bit_equal(got, ref, dt, f"{name} {fdt}->{odt}")
    assert torch.all(cb(far, out_dtype=dt) == 0)
    assert torch.all(torch.isnan(cb(c2, out_dtype=dt)[0, :, 3, 5]))
    assert not torch.isnan(cb(c2, out_dtype=dt)[0, :, 3, 6]).any()
    assert torch.all(torch.isnan(cb(c3, out_dtype=dt)[0, :, 0, 0]))
    o4 = cb(c4, out_dtype=dt)
    assert torch.all(torch.isnan(o4[0, :, 3, 5])) and torch.all(torch.isnan(o4[0, :, 7, 7]))
    assert torch.isfinite(o4[0, :, 3, 6]).all() and (o4[0, :, 3, 6] != 0).any()


# ------------------------- 4. no stray bytes, bare 2-byte alignment (C-ABI)
SENTINEL = 0x5A5A


@pytest.mark.parametrize("flag", ["f16", "bf16"])
@pytest.mark.parametrize("offset", [33, 64])
@pytest.mark.parametrize("case", ["a", "b"])
def test_out16_writes_only_its_elements(dx, case, offset, flag):
    """dxr_corr_lookup into a view of a larger 16-bit buffer that starts at an odd
    element (2-byte aligned only; 64: the aligned control).  The guard elements
    before and after keep their sentinel, the payload is the reference."""
    from dexiraft_amd import _native as nat
    B, D, H, W = CASES[case]
    cb = _block(case, "f32")
    c = _coords(case)
    ref = cb(c)
    n = ref.numel()
    pad = 96
    big = torch.full((offset + n + pad,), SENTINEL, dtype=torch.int16, device=DEV)
    ptr = big.data_ptr() + 2 * offset
    assert ptr % 2 == 0 and (ptr % 4 == 2) == (offset % 2 == 1)
    code = nat.DXR_F32 | (nat.DXR_OUT_F16 if flag == "f16" else nat.DXR_OUT_BF16)
    st = nat.load().dxr_corr_lookup(cb._buf.data_ptr(), code, B, H, W, 4, 4, c.data_ptr(), ptr,
                                    nat.stream_of(c))
    assert st == nat.DXR_OK
    torch.cuda.synchronize()
    assert torch.all(big[:offset] == SENTINEL), "bytes before the output were written"
    assert torch.all(big[offset + n:] == SENTINEL), "bytes after the output were written"
    got = big[offset:offset + n].clone().view(OUT[flag]).reshape(ref.shape)
    assert_bit_equal(got, ref, OUT[flag], f"{case} offset {offset} {flag}")
    # every element was written: the payload's sentinel count is the reference's
    want = ref.to(OUT[flag]).view(torch.int16)
    assert int((big[offset:offset + n] == SENTINEL).sum().item()) == int((want == SENTINEL).sum().item())


# --------------------------------------------------------- 5. lookup_conv1x1
# n: level 3 is 1 x 1, so every lookup vector holds NaNs and every output is NaN (as
# the reference); o: odd N = 323 with finite outputs
CONV_CASES = {"m": (1, 256, 16, 24), "n": (1, 64, 9, 13), "o": (1, 64, 17, 19)}


@lru_cache(maxsize=None)
def _conv_setup(case: str, r: int, cout: int, fdt: str):
    import dexiraft_amd
    B, D, H, W = CONV_CASES[case]
    f1 = _t(dg.fmap(1850, B, D, H, W, "fnet")).to(FMAP[fdt])
    f2 = _t(dg.fmap(1851, B, D, H, W, "fnet")).to(FMAP[fdt])
    with torch.no_grad():
        cb = dexiraft_amd.CorrBlock(f1, f2, radius=r)
    c = _t(dg.coords(1852, B, H, W, "uniform", 6.0))
    w, b = dg.conv1x1_weights(3, cout, 4 * (2 * r + 1) ** 2)
    return cb, c, _t(w), _t(b)


@pytest.mark.parametrize("odt", ["f16", "bf16"])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("case,r,cout,fdt", [("m", 4, 96, "f32"), ("m", 3, 96, "f32"),
                                             ("n", 4, 96, "f32"), ("n", 3, 96, "f32"),
                                             ("n", 4, 256, "f32"), ("o", 4, 96, "f32"),
                                             ("o", 3, 96, "f32"), ("o", 4, 256, "f32"),
                                             ("m", 4, 96, "bf16"), ("o", 3, 96, "bf16")])
def test_out16_lookup_conv1x1(dx, case, r, cout, fdt, relu, odt):
    cb, c, w, b = _conv_setup(case, r, cout, fdt)
    with torch.no_grad():
        ref = cb.lookup_conv1x1(c, w, b, relu=relu)
        got = cb.lookup_conv1x1(c, w, b, relu=relu, out_dtype=OUT[odt])
        assert ref.dtype == torch.float32 and ref.shape == (1, cout) + CONV_CASES[case][2:]
        assert_bit_equal(got, ref, OUT[odt], f"conv {case} r{r} cout{cout} {fdt} relu={relu} ->{odt}")
        if case == "n":
            assert torch.isnan(ref).all()
        else:
            assert torch.isfinite(ref).all()
            assert bool((got < 0).any()) == (not relu)
        # no bias
        assert_bit_equal(cb.lookup_conv1x1(c, w, None, relu=relu, out_dtype=OUT[odt]),
                         cb.lookup_conv1x1(c, w, None, relu=relu), OUT[odt], "no bias")


def test_out16_lookup_conv1x1_bad_dtype(dx):
    cb, c, w, b = _conv_setup("m", 4, 96, "f32")
    with pytest.raises(ValueError, match="float16"):
        cb.lookup_conv1x1(c, w, b, out_dtype=torch.float64)
    with torch.no_grad():
        assert torch.equal(cb.lookup_conv1x1(c, w, b, out_dtype=torch.float32),
                           cb.lookup_conv1x1(c, w, b))


# ------------------------------------------------------------------ 6. autograd
@pytest.mark.parametrize("odt", ["f16", "bf16"])
def test_out16_autograd_matches_f32_output(dx, odt):
    """The backward of a 16-bit lookup is the float32 lookup's on grad_out.float():
    with weights that are exact in the 16-bit type both blocks see the same
    grad_out, so the fmap gradients are equal bit for bit."""
    B, D, H, W = 1, 64, 12, 16
    dt = OUT[odt]
    f1n, f2n = dg.fmap(1860, B, D, H, W, "fnet"), dg.fmap(1861, B, D, H, W, "fnet")
    c = _t(dg.coords(1862, B, H, W, "normal", 4.0))
    w = _t(dg.fmap(1863, B, 4 * 81, H, W, "normal")).to(dt).float()   # exact in dt

    def grads(out_dtype):
        f1, f2 = _t(f1n).requires_grad_(True), _t(f2n).requires_grad_(True)
        cb = dx.CorrBlock(f1, f2)
        out = cb(c) if out_dtype is None else cb(c, out_dtype=out_dtype)
        assert out.requires_grad and out.grad_fn is not None
        assert out.dtype == (torch.float32 if out_dtype is None else out_dtype)
        (out.float() * w).sum().backward()
        return f1.grad, f2.grad, out.detach()

    g1, g2, o32 = grads(None)
    h1, h2, o16 = grads(dt)
    assert_bit_equal(o16, o32, dt, f"grad-mode forward ->{odt}")
    assert g1 is not None and g1.abs().max().item() > 0
    assert torch.equal(g1, h1) and torch.equal(g2, h2)


# ----------------------------------------------------------------- 7. interface
def test_out16_interface(dx):
    cb = _block("c", "f32")
    c = _coords("c")
    for bad in (torch.float64, torch.int16, "float16", 16):
        with pytest.raises(ValueError, match="float16"):
            cb(c, out_dtype=bad)
    a, b = cb(c, out_dtype=torch.float32), cb(c, out_dtype=None)
    assert a.dtype == b.dtype == torch.float32
    assert torch.equal(a, b) and torch.equal(a, cb(c))
    assert a.data_ptr() != b.data_ptr()
    # keyword or positional
    assert torch.equal(_bits(cb(c, torch.float16)), _bits(cb(c, out_dtype=torch.float16)))
    # a block that tracks gradients: no graph under no_grad
    f1, f2 = _fmaps("c", "f32")
    g = dx.CorrBlock(f1.clone().requires_grad_(True), f2.clone().requires_grad_(True))
    assert g(c, out_dtype=torch.float16).grad_fn is not None
    with torch.no_grad():
        o = g(c, out_dtype=torch.float16)
    assert o.grad_fn is None and not o.requires_grad and o.dtype == torch.float16
    assert_bit_equal(o, cb(c), torch.float16, "grad block under no_grad")
    # the alternate block's lookup is unchanged: no out_dtype
    ab = dx.AlternateCorrBlock(*_fmaps("c", "f32"))
    with pytest.raises(TypeError):
        ab(_coords("c"), out_dtype=torch.float16)


# ------------------------------------------------------------- 8. graph capture
def test_out16_graph_replay_matches_eager(dx):
    """A captured build + two float16-output lookups replays to the eager bits
    (tests/test_gpu_graph.py's check for the float32 lookup)."""
    B, D, H, W = 1, 256, 32, 48
    f1 = _t(dg.fmap(1871, B, D, H, W, "fnet"))
    f2 = _t(dg.fmap(1872, B, D, H, W, "fnet"))
    cs = [_t(dg.coords(1873 + k, B, H, W, "normal", 4.0)) for k in range(2)]
    state = {}

    def step():
        blk = dx.CorrBlock(f1, f2, radius=4)
        state["outs"] = [blk(c, out_dtype=torch.float16) for c in cs]
        state["f32"] = [blk(c) for c in cs]

    stream = torch.cuda.Stream(device=DEV)
    with torch.no_grad(), torch.cuda.stream(stream):
        step()
        ref = [o.clone() for o in state["outs"]]
        for o, o32 in zip(ref, state["f32"]):
            assert_bit_equal(o, o32, torch.float16, "eager")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            step()
        for _ in range(3):
            for o in state["outs"]:
                o.zero_()
            g.replay()
            stream.synchronize()
            for a, b in zip(state["outs"], ref):
                assert a.dtype == torch.float16
                assert torch.equal(_bits(a), _bits(b))
