"""GPU: channels-last lookup outputs (``memory_format=torch.channels_last`` of
CorrBlock.__call__ and lookup_conv1x1; DXR_OUT_NHWC at the C-ABI).

The contract is "the same elements at other addresses": every element of the
channels-last result is the NCHW call's element with the same ``out_dtype``, bit
for bit (NaN levels, far and non-finite coordinates, float16 overflow included),
and no byte outside the B*H*W*C elements is written.  So the reference everywhere
is the NCHW call of the same block, every comparison is on the raw bits
(``view(torch.int32)`` / ``view(torch.int16)``), and there is no tolerance.

Shapes are the smallest that reach each code path (D = 32: trivial builds):

  A  B=1  5x7    N = 35: a ragged last workgroup in the 16-query (r <= 4) and the
                 32-/16-query forms; 2 levels, and 3 (the third is 1x1: all NaN);
                 every radius 0-8 (r = 7 / 8 run phase 2 in several passes)
  B  B=3  46x62  N = 2,852, N % 32 = 4; ceil(N/32) * 4 * 3 = 1,080 > 1,024
                 workgroups: the multi-round 512 x 32 shape at r <= 4
  C  B=1  32x32  5 levels: a row-major fifth level

Coordinates are datagen's uniform(-6, 6) displacements (windows partly off the
map) with NaN, +-inf, 1e9 and far-away entries dropped in.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest
import torch

import datagen as dg

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CL = torch.channels_last
SHAPES = {"A": (1, 32, 5, 7), "B": (3, 32, 46, 62), "C": (1, 32, 32, 32)}
SEEDS = {"A": 2110, "B": 2120, "C": 2130}
OUT = {"f32": None, "f16": torch.float16, "bf16": torch.bfloat16}
OUT_TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
PYRS = ("f32", "bf16", "pyr16")   # float32 fmaps, bfloat16 fmaps, float16 fmaps + float16 pyramid

# (shape, radius, num_levels).  Every radius 0-8 on A (r <= 4: the 256 x 16 shape; r = 7 / 8:
# phase 2 in 2 / 4 passes through the smaller staging area, NhwcCfg::PASSES), every radius 0-4
# in the 512 x 32 shape on B: the equality of NaN bits holds per kernel instantiation (the NCHW
# sums' operand order is the compiler's), so each one is compared.
LOOKUPS = ([("A", r, L) for r in range(9) for L in (2, 3)]
           + [("B", r, 4) for r in range(5)] + [("C", 4, 5)])


@pytest.fixture(scope="module")
def dx():
    import dexiraft_amd
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    dexiraft_amd.load_native()
    return dexiraft_amd


def _t(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@lru_cache(maxsize=None)
def _fmaps(shape: str):
    B, D, H, W = SHAPES[shape]
    s = SEEDS[shape]
    return _t(dg.fmap(s, B, D, H, W, "fnet")), _t(dg.fmap(s + 1, B, D, H, W, "fnet"))


@lru_cache(maxsize=None)
def _block(shape: str, pyr: str, r: int, levels: int):
    """One block per configuration, shared by the tests (never modified)."""
    import dexiraft_amd
    f1, f2 = _fmaps(shape)
    with torch.no_grad():
        if pyr == "bf16":
            return dexiraft_amd.CorrBlock(f1.bfloat16(), f2.bfloat16(), num_levels=levels, radius=r)
        if pyr == "pyr16":
            return dexiraft_amd.CorrBlock(f1.half(), f2.half(), num_levels=levels, radius=r,
                                          pyramid_dtype=torch.float16)
        return dexiraft_amd.CorrBlock(f1, f2, num_levels=levels, radius=r)


@lru_cache(maxsize=None)
def _coords(shape: str, k: int = 0):
    B, D, H, W = SHAPES[shape]
    c = dg.coords(SEEDS[shape] + 2 + k, B, H, W, "uniform", 6.0)
    far = dg.coords(SEEDS[shape] + 7, B, H, W, "far")
    c[0, 0, 3, 5] = np.nan
    c[0, 1, 0, 0] = np.inf
    c[0, 0, 4, 6] = -np.inf
    c[0, :, 2, 2] = 1.0e9
    c[0, :, 1, 3] = far[0, :, 1, 3]
    c[B - 1, :, H - 1, W - 1] = far[B - 1, :, H - 1, W - 1]   # the last query of the ragged block
    return _t(c)


def _bits(t: torch.Tensor) -> torch.Tensor:
    """The raw bits of t in NCHW order."""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def assert_same_bits(got: torch.Tensor, ref: torch.Tensor, what: str):
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    gb, rb = _bits(got), _bits(ref)
    bad = gb != rb
    nbad = int(bad.sum().item())
    if nbad:
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {nbad} of {bad.numel()} elements differ; first at {i}: got "
                             f"{gb[i].item():#x}, want {rb[i].item():#x}")


def assert_channels_last(t: torch.Tensor, what: str):
    assert t.is_contiguous(memory_format=CL), what
    B, C, H, W = t.shape
    assert t.permute(0, 2, 3, 1).is_contiguous(), what
    assert t.stride() == (H * W * C, 1, W * C, C), what


def _rounded_buffer(shape: str, pyr: str, r: int, levels: int):
    """A bfloat16 / float16 pyramid of more than 4 levels, which CorrBlock does not
    build (its 16-bit builds stop at the four fused levels): the float32 block's
    paged buffer rounded to that type (same element layout).  Only the lookups'
    two layouts are compared on it, through the C-ABI."""
    from dexiraft_amd import _native as nat
    buf = _block(shape, "f32", r, levels)._buf
    if pyr == "bf16":
        return buf.bfloat16(), nat.DXR_BF16
    return buf.half(), nat.DXR_PYR_F16


def _abi_lookup(pyr_buf, pyr_dt, shape, r, levels, c, odt, nhwc):
    from dexiraft_amd import _native as nat
    B, D, H, W = SHAPES[shape]
    C = levels * (2 * r + 1) ** 2
    flag = {"f32": 0, "f16": nat.DXR_OUT_F16, "bf16": nat.DXR_OUT_BF16}[odt]
    out = torch.empty((B, H, W, C) if nhwc else (B, C, H, W), dtype=OUT_TORCH[odt], device=DEV)
    st = nat.load().dxr_corr_lookup(pyr_buf.data_ptr(), pyr_dt | flag | (nat.DXR_OUT_NHWC if nhwc else 0),
                                    B, H, W, levels, r, c.data_ptr(), out.data_ptr(), nat.stream_of(c))
    assert st == nat.DXR_OK
    return out.permute(0, 3, 1, 2) if nhwc else out


# ------------------------------------------------------------ 1. lookup parity
@pytest.mark.parametrize("odt", list(OUT))
@pytest.mark.parametrize("pyr", PYRS)
@pytest.mark.parametrize("shape,r,levels", LOOKUPS)
def test_channels_last_lookup_equals_nchw(dx, shape, r, levels, pyr, odt):
    B, D, H, W = SHAPES[shape]
    C = levels * (2 * r + 1) ** 2
    c = _coords(shape)
    what = f"{shape} r{r} L{levels} {pyr}->{odt}"
    if pyr != "f32" and levels > 4:
        buf, pyr_dt = _rounded_buffer(shape, pyr, r, levels)
        ref = _abi_lookup(buf, pyr_dt, shape, r, levels, c, odt, False)
        got = _abi_lookup(buf, pyr_dt, shape, r, levels, c, odt, True)
    else:
        cb = _block(shape, pyr, r, levels)
        assert cb._buf.dtype == {"f32": torch.float32, "bf16": torch.bfloat16,
                                 "pyr16": torch.float16}[pyr]
        ref = cb(c, out_dtype=OUT[odt])
        got = cb(c, out_dtype=OUT[odt], memory_format=CL)
        assert ref.is_contiguous()
    assert got.shape == (B, C, H, W) and got.dtype == OUT_TORCH[odt], what
    assert_channels_last(got, what)
    assert_same_bits(got, ref, what)
    # the comparison saw data: finite non-zero values, and NaNs (non-finite coordinates)
    assert (torch.isfinite(ref) & (ref != 0)).any() and torch.isnan(ref).any(), what
    if shape == "A" and levels == 3:
        assert torch.isnan(ref[:, 2 * (2 * r + 1) ** 2:]).all()   # the 1x1 level


# ----------------------------------------------------------- 2. no stray writes
CANARY = 0xA5


@pytest.mark.parametrize("odt", list(OUT))
@pytest.mark.parametrize("shape,r,levels", [("A", 4, 2), ("A", 0, 2), ("B", 4, 4),
                                            ("A", 7, 2), ("A", 8, 2)])   # 7 / 8: the multi-pass phase 2
def test_channels_last_lookup_writes_only_its_elements(dx, shape, r, levels, odt):
    """dxr_corr_lookup | DXR_OUT_NHWC into the interior of a canary-filled byte
    buffer, one element past a 64-byte boundary (16-bit outputs: 2-byte aligned
    only).  Every byte outside the B*H*W*C elements keeps its canary; inside are
    the NCHW call's elements."""
    from dexiraft_amd import _native as nat
    B, D, H, W = SHAPES[shape]
    C = levels * (2 * r + 1) ** 2
    cb = _block(shape, "f32", r, levels)
    c = _coords(shape)
    ref = cb(c, out_dtype=OUT[odt])
    es = ref.element_size()
    n = ref.numel() * es
    off, pad = 64 + es, 4096
    big = torch.full((off + n + pad,), CANARY, dtype=torch.uint8, device=DEV)
    ptr = big.data_ptr() + off
    assert big.data_ptr() % 64 == 0 and ptr % es == 0 and ptr % (2 * es) != 0
    flag = {"f32": 0, "f16": nat.DXR_OUT_F16, "bf16": nat.DXR_OUT_BF16}[odt]
    st = nat.load().dxr_corr_lookup(cb._buf.data_ptr(), nat.DXR_F32 | flag | nat.DXR_OUT_NHWC, B, H, W,
                                    levels, r, c.data_ptr(), ptr, nat.stream_of(c))
    assert st == nat.DXR_OK
    torch.cuda.synchronize()
    assert torch.all(big[:off] == CANARY), "bytes before the output were written"
    assert torch.all(big[off + n:] == CANARY), "bytes after the output were written"
    got = big[off:off + n].clone().view(OUT_TORCH[odt]).reshape(B, H, W, C).permute(0, 3, 1, 2)
    assert_same_bits(got, ref, f"{shape} r{r} {odt} canary")


# ------------------------------------------------------------ 3. fused call
CONV_LEVELS = {"A": 2, "B": 4}


@lru_cache(maxsize=None)
def _conv_weights(r: int, cout: int, levels: int):
    w, b = dg.conv1x1_weights(40 + r, cout, levels * (2 * r + 1) ** 2)
    return _t(w), _t(b)


def _conv_pair(shape, pyr, r, cout, bias, relu, odt):
    cb = _block(shape, pyr, r, CONV_LEVELS[shape])
    w, b = _conv_weights(r, cout, CONV_LEVELS[shape])
    c = _coords(shape)
    with torch.no_grad():
        ref = cb.lookup_conv1x1(c, w, b if bias else None, relu=relu, out_dtype=OUT[odt])
        got = cb.lookup_conv1x1(c, w, b if bias else None, relu=relu, out_dtype=OUT[odt],
                                memory_format=CL)
    return got, ref


@pytest.mark.parametrize("odt", list(OUT))
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("r,cout", [(4, 256), (3, 96)])
@pytest.mark.parametrize("shape", ["A", "B"])   # A: the 1,024-thread form; B: 270 workgroups, 512 threads
def test_channels_last_conv1x1_equals_nchw(dx, shape, r, cout, bias, relu, odt):
    B, D, H, W = SHAPES[shape]
    got, ref = _conv_pair(shape, "f32", r, cout, bias, relu, odt)
    what = f"{shape} r{r} cout{cout} bias{bias} relu{relu} {odt}"
    assert ref.is_contiguous() and ref.shape == (B, cout, H, W)
    assert got.dtype == OUT_TORCH[odt]
    assert_channels_last(got, what)
    assert_same_bits(got, ref, what)
    assert (torch.isfinite(ref) & (ref != 0)).any() and torch.isnan(ref).any(), what


@pytest.mark.parametrize("odt", ["f32", "f16"])
@pytest.mark.parametrize("pyr", ["bf16", "pyr16"])
@pytest.mark.parametrize("shape", ["A", "B"])
def test_channels_last_conv1x1_other_cell_types(dx, shape, pyr, odt):
    got, ref = _conv_pair(shape, pyr, 4, 256, True, True, odt)
    assert_channels_last(got, f"{shape} {pyr} {odt}")
    assert_same_bits(got, ref, f"{shape} {pyr} {odt}")


# -------------------------------------------------------------- 4. autograd
def test_channels_last_lookups_under_autograd(dx):
    B, D, H, W = SHAPES["A"]
    f1, f2 = _fmaps("A")
    cs = [_coords("A", 0), _coords("A", 1)]
    C = 2 * 81
    ws = [_t(dg.fmap(2150 + k, B, C, H, W)) for k in range(2)]   # fixed NCHW weights

    def grads(fmt):
        a, b = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
        cb = dx.CorrBlock(a, b, num_levels=2, radius=4)
        outs = [cb(c, memory_format=fmt) for c in cs]
        for o in outs:
            assert o.requires_grad and o.grad_fn is not None
            if fmt is CL:
                assert_channels_last(o, "under grad")
        # the non-finite coordinates' outputs are NaN: keep them out of the loss
        loss = sum((torch.nan_to_num(o, nan=0.0) * w).sum() for o, w in zip(outs, ws))
        loss.backward()
        return [o.detach() for o in outs], a.grad, b.grad

    o0, ga0, gb0 = grads(None)
    o1, ga1, gb1 = grads(CL)
    for x, y in zip(o1, o0):
        assert_same_bits(x, y, "forward under grad")
    assert torch.isfinite(ga0).all() and (ga0 != 0).any() and (gb0 != 0).any()
    assert_same_bits(ga1, ga0, "d loss / d fmap1")
    assert_same_bits(gb1, gb0, "d loss / d fmap2")
    with torch.no_grad():
        a = f1.clone().requires_grad_(True)
        o = dx.CorrBlock(a, f2, num_levels=2, radius=4)(cs[0], memory_format=CL)
    assert not o.requires_grad and o.grad_fn is None
    assert_channels_last(o, "no_grad")
    assert_same_bits(o, o0[0], "no_grad forward")


# --------------------------------------------------------- 5. graph capture
def test_channels_last_lookups_in_a_graph(dx):
    f1, f2 = _fmaps("A")
    cs = [_coords("A", 0), _coords("A", 1)]
    state = {}

    def step():
        cb = dx.CorrBlock(f1, f2, num_levels=2, radius=4)
        state["outs"] = [cb(c, memory_format=CL) for c in cs]

    stream = torch.cuda.Stream(device=DEV)
    with torch.no_grad(), torch.cuda.stream(stream):
        step()
        stream.synchronize()
        ref = [o.clone() for o in state["outs"]]
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            step()
        for _ in range(2):
            for o in state["outs"]:
                o.zero_()
            g.replay()
            stream.synchronize()
            for a, b in zip(state["outs"], ref):
                assert_channels_last(a, "replay")
                assert_same_bits(a, b, "graph replay vs eager")
    for a, c in zip(ref, cs):
        assert_same_bits(a, _block("A", "f32", 4, 2)(c), "eager channels-last vs NCHW")


# ------------------------------------------------------------ 6. loud paths
def test_bad_memory_format_raises_before_any_launch(dx, monkeypatch):
    from dexiraft_amd import _native as nat
    cb = _block("A", "f32", 4, 2)
    c = _coords("A")
    w, b = _conv_weights(4, 256, 2)

    def no_launch(*a, **k):
        raise AssertionError("the native library was reached")

    monkeypatch.setattr(nat, "load", no_launch)
    for bad in (torch.channels_last_3d, torch.preserve_format, "channels_last", 2):
        with pytest.raises(ValueError, match="channels_last"):
            cb(c, memory_format=bad)
        with pytest.raises(ValueError, match="channels_last"):
            cb.lookup_conv1x1(c, w, b, memory_format=bad)


def test_alternate_block_rejects_the_keyword(dx):
    f1, f2 = _fmaps("C")
    ab = dx.AlternateCorrBlock(f1, f2)
    with pytest.raises(TypeError):
        ab(_coords("C"), memory_format=CL)


def test_default_output_is_still_nchw(dx):
    """None and torch.contiguous_format: a contiguous NCHW float32 tensor, the same
    bits either way, within test_gpu_parity's float32 tolerance of the oracle."""
    import oracle
    from conftest import tolerance_check
    from test_gpu_parity import RTOL
    B, D, H, W = SHAPES["C"]
    f1 = dg.fmap(SEEDS["C"], B, D, H, W, "fnet")
    f2 = dg.fmap(SEEDS["C"] + 1, B, D, H, W, "fnet")
    c = dg.coords(SEEDS["C"] + 9, B, H, W, "uniform", 6.0)
    cb = _block("C", "f32", 4, 5)
    out = cb(_t(c))
    assert out.is_contiguous() and out.dtype == torch.float32 and out.shape == (B, 5 * 81, H, W)
    assert_same_bits(cb(_t(c), memory_format=torch.contiguous_format), out, "contiguous_format")
    assert_same_bits(cb(_t(c), memory_format=CL), out, "channels_last")
    ref = oracle.corr_lookup(oracle.corr_pyramid(f1, f2, 5, np.float64), c, 4)
    tolerance_check(out.cpu().numpy(), ref, RTOL)
