"""GPU: AlternateCorrBlock on float16 feature maps read in place (DXR_ALT_IN_F16).

The contract: with float16 fmaps the block, and the three on-the-fly lookups
with the flag, return what they return on the widened float32 copies of the
fmaps — equal as values with finite fmaps, under every output flag, with and
without coarse volumes — while the block holds float16 operands only.  The
expected tensors therefore come from the float32 path on the widened values;
the float64 oracle of tests/test_gpu_alt_oracle.py (criteria 1-3 of its
docstring, the same BOUND) is applied to the float16 forms as well, and alone
decides where the fmaps hold inf / NaN: there a chunk of the widened path is
recomputed on its bf16 split and value equality is not required.

Shapes, coordinate sets, guard and sentinel are test_gpu_alt_oracle.py's: the
smallest at which ragged tiles, the XCD remainder branch, the prefetch ring
(k-step counts 1, 3, 5 and 16 against a ring of 4) and the ordering kernels'
two-tiles-per-block form can go wrong.
"""
from __future__ import annotations

import ctypes
from functools import lru_cache

import numpy as np
import pytest
import torch

import datagen as dg
import oracle
from test_gpu_alt_oracle import (BOUND, GUARD, SENTINEL, SHAPES, _seed, _t, check_outputs,
                                 coord_set)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ENTRIES = ("lookup", "lookup_ws", "levels_ws")
F16, BF16, NHWC, IN16 = 0x100, 0x200, 0x1000, 0x8000


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
@lru_cache(maxsize=4)
def fmaps16(shape: str, D: int, scaled: bool = False):
    """[B, D, H, W] float32 arrays whose values are float16 numbers, read-only.
    scaled: channels 0-1 of both maps times 2^-20 (float16 subnormals), 2-3 of
    both times 2^14 and clipped to +-6e4 (next to float16's largest, 65504),
    channel 4 small in fmap1 and large in fmap2."""
    B, H, W, _ = SHAPES[shape]
    out = []
    for k in (1, 2):
        f = dg.fmap(_seed("f16", shape, D, k), B, D, H, W).astype(np.float64)
        if scaled:
            f[:, 0:2] *= 2.0 ** -20
            f[:, 2:4] = np.clip(f[:, 2:4] * 2.0 ** 14, -6.0e4, 6.0e4)
            f[:, 4] = f[:, 4] * 2.0 ** -20 if k == 1 else np.clip(f[:, 4] * 2.0 ** 14, -6e4, 6e4)
        h = f.astype(np.float16)
        assert np.isfinite(h).all()
        if scaled:
            tiny = np.abs(h[:, 0:2].astype(np.float64))
            assert ((tiny > 0) & (tiny < 2.0 ** -14)).any(), "no float16 subnormal"
            assert (np.abs(h[:, 2:4].astype(np.float64)) > 5.0e4).any()
        a = h.astype(np.float32)
        a.flags.writeable = False
        out.append(a)
    return tuple(out)


class Operands:
    """NHWC operands of a case on the device: float16 fmap1 / level 0 with the
    float32 pooled levels (the existing pool on the widened level 0), and the
    widened float32 set."""

    def __init__(self, f1: np.ndarray, f2: np.ndarray, L: int):
        from dexiraft_amd import corr
        self.w1 = _t(np.ascontiguousarray(f1.transpose(0, 2, 3, 1)))
        self.w2 = [_t(np.ascontiguousarray(f2.transpose(0, 2, 3, 1)))]
        for _ in range(1, L):
            self.w2.append(corr._pool_nhwc(self.w2[-1]))
        self.h1 = self.w1.half()
        self.h2 = [self.w2[0].half()] + self.w2[1:]
        # exact: the inputs are float16 numbers (or inf / NaN)
        assert torch.equal(torch.nan_to_num(self.h1.float()), torch.nan_to_num(self.w1))
        assert torch.equal(torch.nan_to_num(self.h2[0].float()), torch.nan_to_num(self.w2[0]))
        for t in [self.w1, self.h1] + self.w2 + self.h2:
            assert t.data_ptr() % 16 == 0 and t.is_contiguous()
        self.wptrs = (ctypes.c_void_p * L)(*[t.data_ptr() for t in self.w2])
        self.hptrs = (ctypes.c_void_p * L)(*[t.data_ptr() for t in self.h2])


@lru_cache(maxsize=2)
def operands(shape: str, D: int, scaled: bool = False) -> Operands:
    f1, f2 = fmaps16(shape, D, scaled)
    return Operands(f1, f2, SHAPES[shape][3])


def lookup(entry: str, ops: Operands, native: bool, c: torch.Tensor, shape: str, D: int, r: int,
           flags: int = 0) -> torch.Tensor:
    """One request into a sentinel-filled, guarded float32 buffer (16-bit outputs
    fill its first half); returns the whole buffer."""
    nat = _nat()
    lib = nat.load()
    B, H, W, L = SHAPES[shape]
    K = L * (2 * r + 1) ** 2
    buf = torch.full((B * K * H * W + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    f1, ptrs = (ops.h1, ops.hptrs) if native else (ops.w1, ops.wptrs)
    rad = r | flags | (IN16 if native else 0)
    args = (f1.data_ptr(), ptrs, c.data_ptr(), buf.data_ptr(), B, H, W, D, L)
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
    nat.check(st, f"{entry} native={native} flags={flags:#x}")
    torch.cuda.synchronize()
    return buf


def output_of(buf: torch.Tensor, shape: str, r: int) -> torch.Tensor:
    """The float32 NCHW output of a guarded buffer, after checking the guard."""
    B, H, W, L = SHAPES[shape]
    n = B * L * (2 * r + 1) ** 2 * H * W
    assert (buf[n:] == SENTINEL).all(), "the guard behind the output was written"
    return buf[:n].view(B, -1, H, W)


def equal_values(a: torch.Tensor, b: torch.Tensor) -> bool:
    """torch.equal with NaN where the other has NaN (+0 and -0 are equal)."""
    return bool(torch.equal(torch.isnan(a), torch.isnan(b)) and
                torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0)))


# --------------------------------------------------------------------------- 1. C-ABI, values
POINTS = ([("base", D, 4) for D in (16, 48, 80, 256)] + [("base", 48, r) for r in (0, 3, 6)] +
          [("few", 48, 3), ("tpb2", 80, 4)])
SETS = ("uniform", "integer", "smooth", "nonfinite")
VALUE_RUNS = [p + (s, False) for p in POINTS for s in SETS
              if s != "nonfinite" or SHAPES[p[0]][0] >= 2] + [("base", 48, 4, "uniform", True),
                                                              ("base", 256, 4, "smooth", True)]


@pytest.mark.parametrize("shape,D,r,cset,scaled", VALUE_RUNS,
                         ids=[f"{sh}-D{D}-r{r}-{s}{'-scaled' if sc else ''}"
                              for sh, D, r, s, sc in VALUE_RUNS])
def test_flagged_lookups_equal_the_widened_calls(dx, shape, D, r, cset, scaled):
    B, H, W, L = SHAPES[shape]
    ops = operands(shape, D, scaled)
    c = _t(coord_set(_seed("f16", shape, D, r, cset), cset, B, H, W))
    k = (2 * r + 1) ** 2
    got = {}
    for entry in ENTRIES:
        if entry == "levels_ws" and L < 3:
            continue
        nb = lookup(entry, ops, True, c, shape, D, r)
        wb = lookup(entry, ops, False, c, shape, D, r)
        a, b = output_of(nb, shape, r), output_of(wb, shape, r)
        if cset == "nonfinite":
            assert torch.isnan(b).any()
        else:
            assert torch.isfinite(b[:, :(2 if entry == "levels_ws" else L) * k]).all()
        assert equal_values(a, b), f"{entry}: differs from the unflagged call on widened operands"
        if entry == "levels_ws":
            # levels 2..3 are another request's: they keep the sentinel
            assert (a[:, 2 * k:] == SENTINEL).all() and (a[:, :2 * k] != SENTINEL).any()
        got[entry] = a
    # the ordered and the tile-order float16 forms agree bit for bit
    fin = ~torch.isnan(got["lookup"])
    assert torch.equal(torch.isnan(got["lookup_ws"]), ~fin)
    assert torch.equal(got["lookup"][fin].view(torch.int32), got["lookup_ws"][fin].view(torch.int32))
    if "levels_ws" in got:
        lv, ws = got["levels_ws"][:, :2 * k], got["lookup_ws"][:, :2 * k]
        assert torch.equal(lv[fin[:, :2 * k]].view(torch.int32), ws[fin[:, :2 * k]].view(torch.int32))


# --------------------------------------------------------------------------- 2. flagged outputs
# (r = 6 channels-last: the staged runs of the last phase no longer fit one query plane)
FLAG_RUNS = [("base", 80, 4, F16), ("base", 80, 4, BF16), ("base", 80, 4, NHWC | F16),
             ("base", 80, 4, NHWC | BF16), ("base", 80, 4, NHWC), ("base", 48, 6, NHWC | F16),
             ("base", 48, 6, NHWC)]


@pytest.mark.parametrize("shape,D,r,flags", FLAG_RUNS,
                         ids=[f"{sh}-D{D}-r{r}-{fl:#x}" for sh, D, r, fl in FLAG_RUNS])
def test_output_flags_beside_the_flag_give_the_widened_calls_bits(dx, shape, D, r, flags):
    B, H, W, L = SHAPES[shape]
    ops = operands(shape, D)
    c = _t(coord_set(_seed("f16", shape, D, r, "uniform"), "uniform", B, H, W))
    for entry in ENTRIES:
        nb = lookup(entry, ops, True, c, shape, D, r, flags)
        wb = lookup(entry, ops, False, c, shape, D, r, flags)
        # output, untouched sentinels and the guard alike
        assert torch.equal(nb.view(torch.int32), wb.view(torch.int32)), entry
        assert not torch.equal(nb, torch.full_like(nb, SENTINEL))


# --------------------------------------------------------------------------- 3. float64 oracle
@lru_cache(maxsize=2)
def oracle_reference(shape: str, D: int, r: int, cset: str):
    B, H, W, L = SHAPES[shape]
    f1, f2 = fmaps16(shape, D)
    c = coord_set(_seed("f16", shape, D, r, cset), cset, B, H, W)
    ref = oracle.alt_corr_block(f1, f2, c, L, r, np.float64)
    M = oracle.alt_corr_block(np.abs(f1), np.abs(f2), c, L, r, np.float64)
    return c, ref, M


@pytest.mark.parametrize("D", [48, 256])
def test_float16_forms_match_the_float64_oracle_per_output(dx, D):
    shape, r = "base", 4
    B, H, W, L = SHAPES[shape]
    c, ref, M = oracle_reference(shape, D, r, "uniform")
    ops = operands(shape, D)
    k = (2 * r + 1) ** 2
    for entry in ENTRIES:
        got = output_of(lookup(entry, ops, True, _t(c), shape, D, r), shape, r).cpu().numpy()
        n = 2 if entry == "levels_ws" else L
        check_outputs(f"f16 {entry} D={D}", got[:, :n * k], ref[:, :n * k], M[:, :n * k], n)


def poked_fmaps():
    """("base", 48) with a float16 +inf in one channel of a fmap2 pixel, a NaN in
    another fmap2 pixel and an inf in one fmap1 pixel, all in pair 0 — from level
    1 on every window of r = 4 covers the whole level, so pair 0's coarse outputs
    are non-finite throughout and pair 1 is the finite half — and the same maps
    with those entries 0, for M."""
    f1, f2 = (a.copy() for a in fmaps16("base", 48))
    z1, z2 = f1.copy(), f2.copy()
    f2[0, 5, 2, 17] = np.inf
    f2[0, 11, 16, 1] = np.nan
    f1[0, 7, 9, 4] = -np.inf
    z2[0, 5, 2, 17] = z2[0, 11, 16, 1] = z1[0, 7, 9, 4] = 0.0
    return f1, f2, z1, z2


def check_nonfinite_fmaps(tag: str, got: np.ndarray, ref: np.ndarray, M: np.ndarray) -> None:
    bad = ~np.isfinite(ref)
    assert np.array_equal(~np.isfinite(got), bad), f"{tag}: non-finite where the oracle is not"
    ok = ~bad
    err = np.abs(got[ok].astype(np.float64) - ref[ok])
    assert np.isfinite(M[ok]).all()
    ratio = np.where(M[ok] > 0, err / np.where(M[ok] > 0, M[ok], 1.0), 0.0)
    print(f"ALT-F16 {tag}: {bad.mean():.0%} non-finite, max |err| / M {ratio.max():.3e}")
    assert (got[ok][M[ok] == 0] == 0).all()
    assert (err <= BOUND * M[ok]).all(), f"{tag}: max |err| / M {ratio.max():.3e} > {BOUND}"


def test_nonfinite_fmaps_match_the_float64_oracle(dx):
    """Non-finite exactly where the float64 oracle is (inf or NaN: 0 x inf, inf -
    inf and the oracle's inf are one class), within BOUND M elsewhere, with M
    from the maps with the poked entries 0.  The float16 forms and — so that the
    case asks nothing the widened path does not meet — the unflagged calls on the
    widened maps."""
    shape, D, r = "base", 48, 4
    B, H, W, L = SHAPES[shape]
    f1, f2, z1, z2 = poked_fmaps()
    c = coord_set(_seed("f16", shape, D, r, "uniform"), "uniform", B, H, W)
    with np.errstate(invalid="ignore", over="ignore"):
        ref = oracle.alt_corr_block(f1, f2, c, L, r, np.float64)
    M = oracle.alt_corr_block(np.abs(z1), np.abs(z2), c, L, r, np.float64)
    k = (2 * r + 1) ** 2
    fin = np.isfinite(ref)
    for lvl in range(L):     # the case leaves at least half of every level's outputs finite
        assert fin[:, lvl * k:(lvl + 1) * k].mean() >= 0.5, lvl
    assert not fin.all() and fin[1].all()
    ops = Operands(f1, f2, L)
    for native in (True, False):
        for entry in ENTRIES:
            got = output_of(lookup(entry, ops, native, _t(c), shape, D, r), shape, r).cpu().numpy()
            n = 2 if entry == "levels_ws" else L
            check_nonfinite_fmaps(f"{entry} {'float16' if native else 'widened'}", got[:, :n * k],
                                  ref[:, :n * k], M[:, :n * k])


# --------------------------------------------------------------------------- 4. the class
def _held_bytes(blk) -> int:
    """Bytes of the distinct storages behind the block's tensor attributes."""
    seen = {}

    def visit(v):
        if isinstance(v, torch.Tensor):
            st = v.untyped_storage()
            seen[st.data_ptr()] = st.nbytes()
        elif isinstance(v, (list, tuple)):
            for e in v:
                visit(e)

    for v in vars(blk).values():
        visit(v)
    return sum(seen.values())


def _class_inputs(D: int = 64):
    B, H, W, L = SHAPES["base"]
    f1, f2 = fmaps16("base", D)
    cs = [_t(coord_set(_seed("f16", "class", D, s), s, B, H, W)) for s in ("uniform", "nonfinite")]
    return _t(f1).half(), _t(f2).half(), cs, L


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
@pytest.mark.parametrize("out", [None, (torch.float16, torch.channels_last)])
def test_block_on_float16_fmaps_equals_the_widened_block(dx, layout, out):
    h1, h2, cs, L = _class_inputs()
    if layout == "channels_last":
        h1 = h1.contiguous(memory_format=torch.channels_last)
        h2 = h2.contiguous(memory_format=torch.channels_last)
    kw = {} if out is None else dict(out_dtype=out[0], memory_format=out[1])
    blk = dx.AlternateCorrBlock(h1, h2, L, 4, **kw)
    wide = dx.AlternateCorrBlock(h1.float(), h2.float(), L, 4, **kw)
    # float16 operands in place, float32 pooled levels, no widened copy of the fmaps
    assert blk._f1_nhwc.dtype == torch.float16 and blk._f2_nhwc[0].dtype == torch.float16
    assert all(t.dtype == torch.float32 for t in blk._f2_nhwc[1:])
    assert blk._f2_nhwc[1].dtype == torch.float32 and wide._f1_nhwc.dtype == torch.float32
    for a, b in zip(blk._f2_nhwc[1:], wide._f2_nhwc[1:]):
        assert torch.equal(a, b)
    for c in cs:
        a, b = blk(c), wide(c)
        assert a.dtype == b.dtype and a.stride() == b.stride()
        assert equal_values(a.float(), b.float())
    assert blk._in16, "the library declined the flag"
    # bytes held: E elements per map.  Widened: two float32 fmaps and their float32 NHWC
    # operands (views of channels-last fmaps), 16 E (8 E); float16 in place: the two float16
    # NHWC operands, 4 E — half of the widened block's or less; both hold the pooled levels
    E = h1.numel()
    pooled = sum(t.numel() * 4 for t in wide._f2_nhwc[1:])
    assert _held_bytes(wide) == (8 if layout == "channels_last" else 16) * E + pooled
    assert _held_bytes(blk) == 4 * E + pooled
    assert _held_bytes(blk) - pooled <= 0.5 * (_held_bytes(wide) - pooled)
    # the reference's pyramid: float32, the widened block's values and layouts
    for (a1, a2), (b1, b2) in zip(blk.pyramid, wide.pyramid):
        for a, b in ((a1, b1), (a2, b2)):
            assert a.dtype == torch.float32 and a.shape == b.shape and a.stride() == b.stride()
            assert torch.equal(a, b)


def test_block_with_coarse_volumes_and_without_the_knob(dx, monkeypatch):
    h1, h2, cs, L = _class_inputs()
    wide = dx.AlternateCorrBlock(h1.float(), h2.float(), L, 4)
    want = [wide(c) for c in cs]
    monkeypatch.setattr(dx.AlternateCorrBlock, "NATIVE_F16", False)
    off = dx.AlternateCorrBlock(h1, h2, L, 4)
    assert off._f1_nhwc.dtype == torch.float32 and not off._in16
    for c, w in zip(cs, want):
        assert equal_values(off(c), w)
    monkeypatch.setattr(dx.AlternateCorrBlock, "NATIVE_F16", True)
    monkeypatch.setattr(dx.AlternateCorrBlock, "COARSE_MIN_QUERIES", 0)
    monkeypatch.setattr(dx.AlternateCorrBlock, "COARSE_LEVEL_MAX_CELLS", 1 << 20)
    monkeypatch.setattr(dx.AlternateCorrBlock, "COARSE_VOLUME_MAX_BYTES", 1 << 32)
    vol = dx.AlternateCorrBlock(h1, h2, L, 4)
    wvol = dx.AlternateCorrBlock(h1.float(), h2.float(), L, 4)
    assert vol.coarse_first_level == wvol.coarse_first_level == 1 and vol._in16
    assert vol._f1_nhwc.dtype == torch.float16
    assert torch.equal(vol._volumes, wvol._volumes)
    for c, w in zip(cs, want):
        assert equal_values(vol(c), wvol(c))
        assert equal_values(vol(c), w)


def test_unserved_channel_counts_and_radii_are_widened(dx):
    """D = 40 (a VALU form) and radius 7 take no float16 operands: the constructor
    widens as ever."""
    B, H, W, L = SHAPES["base"]
    f1, f2 = fmaps16("base", 40)
    h1, h2 = _t(f1).half(), _t(f2).half()
    c = _t(coord_set(_seed("f16", "class", 40), "uniform", B, H, W))
    blk = dx.AlternateCorrBlock(h1, h2, L, 3)
    assert blk._f1_nhwc.dtype == torch.float32 and not blk._in16
    assert torch.equal(blk(c), dx.AlternateCorrBlock(h1.float(), h2.float(), L, 3)(c))
    bf = dx.AlternateCorrBlock(h1.bfloat16(), h2.bfloat16(), L, 3)
    assert bf._f1_nhwc.dtype == torch.float32 and not bf._in16


def test_declined_flag_widens_once_and_goes_on(dx):
    """The library answers the flag with DXR_EUNSUPPORTED (here for a float16
    fmap1 that is 8 bytes off 16-byte alignment): the block widens its operands,
    remembers, and returns the widened block's outputs."""
    h1, h2, cs, L = _class_inputs()
    blk = dx.AlternateCorrBlock(h1, h2, L, 4)
    wide = dx.AlternateCorrBlock(h1.float(), h2.float(), L, 4)
    store = torch.empty(blk._f1_nhwc.numel() + 8, dtype=torch.float16, device=DEV)
    off = store[4:4 + blk._f1_nhwc.numel()].view(blk._f1_nhwc.shape)
    off.copy_(blk._f1_nhwc)
    assert off.data_ptr() % 16 == 8
    blk._f1_nhwc = off
    assert equal_values(blk(cs[0]), wide(cs[0]))
    assert not blk._in16 and blk._f1_nhwc.dtype == torch.float32
    assert blk._f2_nhwc[0].dtype == torch.float32
    assert equal_values(blk(cs[1]), wide(cs[1]))


def test_trainable_block_on_float16_fmaps(dx, monkeypatch):
    """Without grad: AlternateCorrBlock's float16 path.  With fmaps that require
    grad: the tracked .float() comes first, so NATIVE_F16 changes nothing — equal
    outputs and gradients.  dfmap1 has a fixed summation order; dfmap2 is summed
    by atomics, whose order moves its last bits from run to run, so it is
    compared where the order cannot matter: a grad_out that is non-zero at one
    query (every other contribution is an exact zero)."""
    h1, h2, cs, L = _class_inputs()
    c = cs[0]
    plain = dx.AlternateCorrBlock(h1, h2, L, 4)(c)
    t = dx.TrainableAlternateCorrBlock(h1, h2, L, 4)
    assert t._in16 and t._f1_nhwc.dtype == torch.float16
    assert equal_values(t(c), plain)
    B, _, H, W = plain.shape
    dense = _t(dg.normal(_seed("f16", "gout"), plain.numel()).reshape(plain.shape).astype(np.float32))
    one = torch.zeros_like(dense)
    one[1, :, H // 2, W // 2] = dense[1, :, H // 2, W // 2]

    def run(native: bool):
        monkeypatch.setattr(dx.AlternateCorrBlock, "NATIVE_F16", native)
        a1, a2 = h1.clone().requires_grad_(True), h2.clone().requires_grad_(True)
        blk = dx.TrainableAlternateCorrBlock(a1, a2, L, 4)
        assert not blk._in16 and blk._f1_nhwc.dtype == torch.float32
        o = blk(c)
        gd = torch.autograd.grad([o], [a1, a2], [dense], retain_graph=True)
        go = torch.autograd.grad([o], [a1, a2], [one])
        return o.detach(), gd, go

    o1, gd1, go1 = run(True)
    o0, gd0, go0 = run(False)
    assert equal_values(o1, o0) and equal_values(o1, plain)
    assert gd1[0].dtype == torch.float16 and gd1[0].abs().max() > 0
    assert torch.equal(gd1[0], gd0[0])
    assert go1[1].abs().max() > 0
    assert torch.equal(go1[0], go0[0]) and torch.equal(go1[1], go0[1])


# --------------------------------------------------------------------------- 5. graph capture
def test_graph_capture_of_float16_lookups_matches_eager(dx):
    """tests/test_gpu_graph.py's pattern on a float16 block: two lookups captured
    once and replayed give the eager outputs."""
    h1, h2, cs, L = _class_inputs()
    state = {}

    def step():
        blk = dx.AlternateCorrBlock(h1, h2, L, 4)
        assert blk._in16
        state["outs"] = [blk(c) for c in cs]

    stream = torch.cuda.Stream(device=DEV)
    with torch.no_grad(), torch.cuda.stream(stream):
        step()
        ref = [o.clone() for o in state["outs"]]
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            step()
        for o in state["outs"]:
            o.zero_()
        g.replay()
        stream.synchronize()
        for a, b in zip(state["outs"], ref):
            assert equal_values(a, b)
