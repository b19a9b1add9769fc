"""GPU: AlternateCorrBlock on bfloat16 feature maps read in place (DXR_ALT_IN_BF16).

Unlike the float16 form (tests/test_gpu_alt_f16.py) this one is not bit-equal to
the block on the widened maps: the same exact products are summed by another
matrix-core instruction.  The contract is therefore the float64 oracle's, per
output, as in tests/test_gpu_alt_oracle.py (criteria 1-5 of its docstring, the
same BOUND = 1e-5: every product here is exact — 8-bit significands, or an
exact three-way split of a float32 cell times an 8-bit significand — so what is
left is the float32 accumulation, the four multiply-adds and the divide that
docstring counts), with the oracle given the widened values, and on top of it:

  - the ordered and the tile-order forms agree bit for bit;
  - every flagged output is the native block's own float32 NCHW output
    converted, bit for bit;
  - the pooled levels and the coarse volumes are the widened block's bit for
    bit (the same calls on the same float32 operands);
  - values outside float16's range on both sides need no other path.

Shapes, coordinate sets, guard and sentinel are test_gpu_alt_oracle.py's: the
smallest at which ragged tiles, the XCD remainder branch, the prefetch ring
(k-step counts 1, 2, 3, 5 and 16 against a ring of 4) and the ordering kernels'
two-tiles-per-block form can go wrong.  No bfloat16 subnormal is fed: how the
bf16 matrix-core instruction treats them is not measured here.
"""
from __future__ import annotations

import ctypes
from functools import lru_cache

import numpy as np
import pytest
import torch

import datagen as dg
import oracle
from test_gpu_alt_oracle import (GUARD, SENTINEL, SHAPES, _seed, _t, check_nonfinite_reference,
                                 check_outputs, coord_set)
from test_gpu_alt_out import KINDS, assert_same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ENTRIES = ("lookup", "lookup_ws", "levels_ws")
F16, BF16, NHWC, INBF = 0x100, 0x200, 0x1000, 0x20000


@pytest.fixture(scope="module")
def dx():
    import dexiraft_amd
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    dexiraft_amd.load_native()
    return dexiraft_amd


def _nat():
    from dexiraft_amd import _native
    return _native


# --------------------------------------------------------------------------- inputs
def to_bf16_values(a: np.ndarray) -> np.ndarray:
    """float32 array rounded (to nearest even) to bfloat16 numbers."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().float().numpy()


@lru_cache(maxsize=4)
def fmaps_bf16(shape: str, D: int, ranged: bool = False):
    """[B, D, H, W] float32 arrays whose values are bfloat16 numbers, read-only.
    ranged: in both maps a quarter of the pixels times 2^20 and a quarter times
    2^-30 — normal bfloat16 numbers outside float16's range on both sides."""
    B, H, W, _ = SHAPES[shape]
    out = []
    for k in (1, 2):
        a = to_bf16_values(dg.fmap(_seed("bf16", shape, D, k), B, D, H, W))
        if ranged:
            pix = (np.arange(H)[:, None] * W + np.arange(W)[None, :] + k) % 4
            a = a * np.where(pix == 0, np.float32(2.0 ** 20),
                             np.where(pix == 1, np.float32(2.0 ** -30), np.float32(1.0)))
            a = a.astype(np.float32)
            mag = np.abs(a)
            assert (mag > 65504.0).any() and ((mag > 0) & (mag < 2.0 ** -24)).any()
        assert np.isfinite(a).all() and np.array_equal(to_bf16_values(a), a)
        mag = np.abs(a)
        assert ((mag == 0) | (mag >= 2.0 ** -126)).all(), "a bfloat16 subnormal"
        a.flags.writeable = False
        out.append(a)
    return tuple(out)


class Operands:
    """NHWC operands of a case on the device: bfloat16 fmap1 / level 0 with the
    float32 pooled levels (the existing pool on the widened level 0)."""

    def __init__(self, f1: np.ndarray, f2: np.ndarray, L: int):
        from dexiraft_amd import corr
        w1 = _t(np.ascontiguousarray(f1.transpose(0, 2, 3, 1)))
        w2 = [_t(np.ascontiguousarray(f2.transpose(0, 2, 3, 1)))]
        lvl = f2
        for i in range(1, L):
            w2.append(corr._pool_nhwc(w2[-1]))
            lvl = oracle.avg_pool2x2(lvl)    # the oracle's float32 pools, bit for bit
            assert np.array_equal(w2[i].cpu().numpy(), lvl.transpose(0, 2, 3, 1)), i
        self.b1 = w1.bfloat16()
        self.b2 = [w2[0].bfloat16()] + w2[1:]
        assert torch.equal(self.b1.float(), w1) and torch.equal(self.b2[0].float(), w2[0])
        for t in [self.b1] + self.b2:
            assert t.data_ptr() % 16 == 0 and t.is_contiguous()
        assert self.b1.dtype == self.b2[0].dtype == torch.bfloat16
        self.ptrs = (ctypes.c_void_p * L)(*[t.data_ptr() for t in self.b2])


@lru_cache(maxsize=2)
def operands(shape: str, D: int, ranged: bool = False) -> Operands:
    f1, f2 = fmaps_bf16(shape, D, ranged)
    return Operands(f1, f2, SHAPES[shape][3])


@lru_cache(maxsize=4)
def reference(shape: str, D: int, r: int, cset: str, ranged: bool = False):
    """(coords, ref, M), read-only: the float64 oracle on the widened values and
    on their absolute values."""
    B, H, W, L = SHAPES[shape]
    f1, f2 = fmaps_bf16(shape, D, ranged)
    c = coord_set(_seed("bf16", shape, D, r, cset), cset, B, H, W)
    with np.errstate(invalid="ignore"):
        ref = oracle.alt_corr_block(f1, f2, c, L, r, np.float64)
        M = oracle.alt_corr_block(np.abs(f1), np.abs(f2), c, L, r, np.float64)
    for a in (c, ref, M):
        a.flags.writeable = False
    return c, ref, M


def lookup(entry: str, ops: Operands, c: torch.Tensor, shape: str, D: int, r: int,
           flags: int = 0) -> torch.Tensor:
    """One flagged request into a sentinel-filled, guarded float32 buffer;
    returns the whole buffer."""
    nat = _nat()
    lib = nat.load()
    B, H, W, L = SHAPES[shape]
    K = L * (2 * r + 1) ** 2
    buf = torch.full((B * K * H * W + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    rad = r | flags | INBF
    args = (ops.b1.data_ptr(), ops.ptrs, c.data_ptr(), buf.data_ptr(), B, H, W, D, L)
    div = float(np.sqrt(np.float32(D), dtype=np.float32))
    s = nat.stream_of(buf)
    if entry == "lookup":
        st = lib.dxr_alt_corr_lookup(*args, rad, div, s)
    else:
        nl = L if entry == "lookup_ws" else 2
        n = lib.dxr_alt_workspace_bytes(B, H, W, nl)
        assert n > 0
        ws = torch.empty(n, dtype=torch.uint8, device=DEV)
        assert ws.data_ptr() % 16 == 0
        if entry == "lookup_ws":
            st = lib.dxr_alt_corr_lookup_ws(*args, rad, div, ws.data_ptr(), n, s)
        else:
            st = lib.dxr_alt_corr_lookup_levels_ws(*args, 2, rad, div, ws.data_ptr(), n, s)
    nat.check(st, f"{entry} flags={flags:#x}")
    torch.cuda.synchronize()
    return buf


def output_of(buf: torch.Tensor, shape: str, r: int) -> np.ndarray:
    """The float32 NCHW output of a guarded buffer, after checking the guard's bits."""
    B, H, W, L = SHAPES[shape]
    n = B * L * (2 * r + 1) ** 2 * H * W
    res = buf.cpu().numpy()
    assert np.array_equal(res[n:].view(np.int32),
                          np.full(GUARD, SENTINEL, np.float32).view(np.int32)), \
        "the guard behind the output was written"
    return res[:n].reshape(B, -1, H, W)


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    """Bit equality with NaNs in place (a NaN's payload is not compared)."""
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and
                np.array_equal(a.view(np.int32)[~na], b.view(np.int32)[~nb]))


def check_case(shape: str, D: int, r: int, cset: str, ranged: bool = False) -> None:
    """Criteria 1-5 on the three entry points with the flag."""
    B, H, W, L = SHAPES[shape]
    c, ref, M = reference(shape, D, r, cset, ranged)
    if cset == "nonfinite":
        check_nonfinite_reference(c, ref)
    ops = operands(shape, D, ranged)
    k = (2 * r + 1) ** 2
    got = {}
    for entry in ENTRIES:
        if entry == "levels_ws" and L < 3:
            continue
        a = output_of(lookup(entry, ops, _t(c), shape, D, r), shape, r)
        tag = f"bf16 {entry} {shape} D={D} r={r} {cset}{' ranged' if ranged else ''}"
        n = L
        if entry == "levels_ws":
            # levels 2..3 are another request's: their channels keep the sentinel's bits
            n = 2
            rest = a[:, 2 * k:]
            assert np.array_equal(rest.view(np.int32),
                                  np.full(rest.shape, SENTINEL, np.float32).view(np.int32)), \
                f"{tag}: a channel of a level that was not requested was written"
        # (asserts, too, that every level has outputs with M > 0)
        check_outputs(tag, a[:, :n * k], ref[:, :n * k], M[:, :n * k], n)
        if ranged:
            assert np.isfinite(a[:, :n * k]).all(), tag
        got[entry] = a
    assert same_bits(got["lookup_ws"], got["lookup"]), "ordered differs from the tile-order form"
    if "levels_ws" in got:
        assert same_bits(got["levels_ws"][:, :2 * k], got["lookup"][:, :2 * k])


# --------------------------------------------------------------------------- 1. C-ABI, values
POINTS = ([("base", 48, r) for r in range(7)] + [("base", D, 4) for D in (16, 32, 80, 256)] +
          [("few", 48, 3), ("tpb2", 80, 4)])
SETS = ("uniform", "integer", "smooth")
VALUE_RUNS = [p + (s,) for p in POINTS
              for s in SETS + (("nonfinite",) if p == ("base", 48, 4) else ())]


@pytest.mark.parametrize("shape,D,r,cset", VALUE_RUNS,
                         ids=[f"{sh}-D{D}-r{r}-{s}" for sh, D, r, s in VALUE_RUNS])
def test_flagged_lookups_match_the_float64_oracle_per_output(dx, shape, D, r, cset):
    check_case(shape, D, r, cset)


# --------------------------------------------------------------------------- 2. range
def test_values_outside_float16s_range_need_no_other_path(dx):
    """A quarter of the pixels times 2^20, a quarter times 2^-30: the same
    criterion, every output finite."""
    check_case("base", 48, 4, "uniform", ranged=True)


# --------------------------------------------------------------------------- 3. the class
def _class_inputs(D: int, shape: str = "base"):
    B, H, W, L = SHAPES[shape]
    f1, f2 = fmaps_bf16(shape, D)
    return _t(f1).bfloat16(), _t(f2).bfloat16(), L


CLASS_RUNS = [(D, r, lay) for D in (64, 256) for r in (3, 4) for lay in ("nchw", "channels_last")]


@pytest.mark.parametrize("D,r,layout", CLASS_RUNS, ids=[f"D{D}-r{r}-{l}" for D, r, l in CLASS_RUNS])
def test_block_on_bfloat16_fmaps(dx, D, r, layout, monkeypatch):
    shape = "base"
    B, H, W, L = SHAPES[shape]
    b1, b2, _ = _class_inputs(D)
    assert b1.dtype == torch.bfloat16
    if layout == "channels_last":
        b1 = b1.contiguous(memory_format=torch.channels_last)
        b2 = b2.contiguous(memory_format=torch.channels_last)
    c, ref, M = reference(shape, D, r, "uniform")
    ct = _t(c)
    blk = dx.AlternateCorrBlock(b1, b2, L, r)
    wide = dx.AlternateCorrBlock(b1.float(), b2.float(), L, r)
    # bfloat16 operands in place, float32 pooled levels: the widened block's bit for bit
    assert blk._f1_nhwc.dtype == blk._f2_nhwc[0].dtype == torch.bfloat16
    assert blk._inbf16 and not blk._in16 and blk._fmaps is None
    assert wide._f1_nhwc.dtype == torch.float32 and not wide._inbf16
    assert len(blk._f2_nhwc) == L
    for a, b in zip(blk._f2_nhwc[1:], wide._f2_nhwc[1:]):
        assert a.dtype == torch.float32 and torch.equal(a, b)
    if layout == "channels_last":   # a free view of the caller's storage
        assert blk._f1_nhwc.data_ptr() == b1.data_ptr()
        assert blk._f2_nhwc[0].data_ptr() == b2.data_ptr()
    base = blk(ct)
    assert blk._inbf16, "the library declined the flag"
    assert base.dtype == torch.float32 and base.is_contiguous()
    check_outputs(f"bf16 block D={D} r={r} {layout}", base.cpu().numpy(), ref, M, L)
    # the reference's pyramid: float32, the widened block's values and layouts
    for (a1, a2), (w1, w2) in zip(blk.pyramid, wide.pyramid):
        for a, b in ((a1, w1), (a2, w2)):
            assert a.dtype == torch.float32 and a.shape == b.shape and a.stride() == b.stride()
            assert torch.equal(a, b)
    # every flagged output: the native block's own float32 NCHW output converted
    K = L * (2 * r + 1) ** 2
    for dt, mf in KINDS:
        ab = dx.AlternateCorrBlock(b1, b2, L, r, out_dtype=dt, memory_format=mf)
        got = ab(ct)
        assert ab._inbf16 and ab._out_native
        tag = f"D={D} r={r} {layout} {dt} {mf}"
        want = base.to(dt or torch.float32)
        assert got.dtype == want.dtype and got.shape == base.shape, tag
        if mf is torch.channels_last:
            assert got.stride() == (H * W * K, 1, W * K, K), tag
            want = want.contiguous(memory_format=torch.channels_last)
            assert_same_bits(got.permute(0, 2, 3, 1), want.permute(0, 2, 3, 1), tag)
        else:
            assert got.is_contiguous(), tag
            assert_same_bits(got, want, tag)
    # without the knob: the widening constructor
    monkeypatch.setattr(dx.AlternateCorrBlock, "NATIVE_BF16", False)
    off = dx.AlternateCorrBlock(b1, b2, L, r)
    assert off._f1_nhwc.dtype == off._f2_nhwc[0].dtype == torch.float32 and not off._inbf16
    assert off._fmaps is not None
    assert torch.equal(off(ct), wide(ct))


# --------------------------------------------------------------------------- 4. coarse volumes
def volume_cells(B: int, H: int, W: int, L: int, first: int) -> np.ndarray:
    """Element indices, in a block's ``_volumes``, of every (pair, query, cell) of
    the levels >= first: the paged layout of csrc/dxr_common.h (make_levels,
    cell_index) — pages of 128 queries x one (8 >> l) x (16 >> l) tile, queries
    padded to whole pages and the level to whole tiles.  The padding belongs to
    no cell; the form that serves D % 32 != 0 never writes it."""
    assert L <= 4
    N = H * W
    qt, ty, tx = -(-N // 128), -(-H // 8), -(-W // 16)
    idx, off, h, w = [], 0, H, W
    for l in range(L):
        if l:
            h, w = h // 2, w // 2
        th, tw = 8 >> l, 16 >> l
        if l >= first:
            b, q, y, x = np.meshgrid(np.arange(B), np.arange(N), np.arange(h), np.arange(w),
                                     indexing="ij")
            page = ((b * qt + q // 128) * ty + y // th) * tx + x // tw
            idx.append((off + (page * 128 + q % 128) * (th * tw) + (y % th) * tw + x % tw).ravel())
            off += B * qt * 128 * ty * tx * th * tw
    idx = np.concatenate(idx)
    assert len(np.unique(idx)) == len(idx) and idx.max() < off
    return idx


def test_block_with_coarse_volumes(dx, monkeypatch):
    shape, D, r = "tpb2", 80, 4
    B, H, W, L = SHAPES[shape]
    b1, b2, _ = _class_inputs(D, shape)
    c, ref, M = reference(shape, D, r, "uniform")
    ct = _t(c)
    assert dx.AlternateCorrBlock(b1, b2, L, r).coarse_first_level is None
    monkeypatch.setattr(dx.AlternateCorrBlock, "COARSE_MIN_QUERIES", 0)
    vol = dx.AlternateCorrBlock(b1, b2, L, r)
    wvol = dx.AlternateCorrBlock(b1.float(), b2.float(), L, r)
    first = vol.coarse_first_level
    assert first is not None and first == wvol.coarse_first_level and 1 <= first < L
    assert vol._inbf16 and vol._f1_nhwc.dtype == torch.bfloat16
    # every cell of the volumes (D = 80 takes the form that leaves the pages' padding
    # unwritten, so the buffers are compared where they hold cells)
    assert vol._volumes.numel() == wvol._volumes.numel() == \
        _nat().load().dxr_alt_volume_numel(B, H, W, L, first)
    cells = torch.from_numpy(volume_cells(B, H, W, L, first)).to(DEV)
    assert int(cells.max()) < vol._volumes.numel()
    va, vb = vol._volumes[cells], wvol._volumes[cells]
    assert torch.isfinite(vb).all() and bool((vb != 0).any())
    assert torch.equal(va, vb)
    a, b = vol(ct), wvol(ct)
    assert vol._inbf16, "the library declined the flag"
    k = (2 * r + 1) ** 2
    # the volume levels: the same call on the same float32 operands
    assert torch.equal(a[:, first * k:], b[:, first * k:])
    got = a.cpu().numpy()
    check_outputs("bf16 volumes: fine levels", got[:, :first * k], ref[:, :first * k],
                  M[:, :first * k], first)
    check_outputs("bf16 volumes: all levels", got, ref, M, L)


# --------------------------------------------------------------------------- 5. fallbacks
def test_unserved_channel_counts_and_radii_are_widened(dx):
    """D = 40 (a VALU form) and radius 7 take no bfloat16 operands: the
    constructor widens as ever."""
    B, H, W, L = SHAPES["base"]
    b1, b2, _ = _class_inputs(40)
    c = _t(coord_set(_seed("bf16", "class", 40), "uniform", B, H, W))
    blk = dx.AlternateCorrBlock(b1, b2, L, 3)
    assert blk._f1_nhwc.dtype == blk._f2_nhwc[0].dtype == torch.float32 and not blk._inbf16
    assert torch.equal(blk(c), dx.AlternateCorrBlock(b1.float(), b2.float(), L, 3)(c))
    b1, b2, _ = _class_inputs(64)
    far = dx.AlternateCorrBlock(b1, b2, L, 7)
    assert far._f1_nhwc.dtype == far._f2_nhwc[0].dtype == torch.float32 and not far._inbf16


def test_declined_flag_widens_once_and_goes_on(dx):
    """The library answers the flag with DXR_EUNSUPPORTED (here for a bfloat16
    fmap1 that is 8 bytes off 16-byte alignment): the block widens its operands,
    remembers, and returns the widened block's outputs."""
    B, H, W, L = SHAPES["base"]
    b1, b2, _ = _class_inputs(64)
    cs = [_t(coord_set(_seed("bf16", "declined", s), s, B, H, W)) for s in ("uniform", "nonfinite")]
    blk = dx.AlternateCorrBlock(b1, b2, L, 4)
    wide = dx.AlternateCorrBlock(b1.float(), b2.float(), L, 4)
    assert blk._inbf16
    store = torch.empty(blk._f1_nhwc.numel() + 8, dtype=torch.bfloat16, device=DEV)
    off = store[4:4 + blk._f1_nhwc.numel()].view(blk._f1_nhwc.shape)
    off.copy_(blk._f1_nhwc)
    assert off.data_ptr() % 16 == 8
    blk._f1_nhwc = off
    for c in cs:
        a, b = blk(c), wide(c)
        assert not blk._inbf16 and not blk._in16
        assert blk._f1_nhwc.dtype == blk._f2_nhwc[0].dtype == torch.float32
        assert torch.equal(torch.isnan(a), torch.isnan(b))
        assert torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0))


def test_trainable_block_inherits_the_native_form_without_grad(dx):
    B, H, W, L = SHAPES["base"]
    b1, b2, _ = _class_inputs(64)
    c = _t(coord_set(_seed("bf16", "train"), "uniform", B, H, W))
    t = dx.TrainableAlternateCorrBlock(b1, b2, L, 4)
    assert t._inbf16 and t._f1_nhwc.dtype == torch.bfloat16
    assert torch.equal(t(c), dx.AlternateCorrBlock(b1, b2, L, 4)(c))
    g = dx.TrainableAlternateCorrBlock(b1.clone().requires_grad_(True), b2, L, 4)
    assert not g._inbf16 and g._f1_nhwc.dtype == torch.float32   # widened before the constructor


# --------------------------------------------------------------------------- 6. graph capture
def test_graph_capture_of_twelve_bfloat16_lookups_matches_eager(dx):
    B, H, W, L = SHAPES["base"]
    b1, b2, _ = _class_inputs(64)
    cs = [_t(coord_set(_seed("bf16", "graph", i), ("uniform", "smooth", "integer")[i % 3], B, H, W))
          for i in range(12)]
    state = {}

    def step():
        blk = dx.AlternateCorrBlock(b1, b2, L, 4)
        assert blk._inbf16
        state["outs"] = [blk(c) for c in cs]
        assert blk._inbf16

    stream = torch.cuda.Stream(device=DEV)
    with torch.no_grad(), torch.cuda.stream(stream):
        step()
        stream.synchronize()
        ref = [o.clone() for o in state["outs"]]
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            step()
        for o in state["outs"]:
            o.zero_()
        g.replay()
        stream.synchronize()
        assert len(ref) == 12
        for a, b in zip(state["outs"], ref):
            assert_same_bits(a, b, "replay")
        assert any(bool(o.abs().max() > 0) for o in ref)
