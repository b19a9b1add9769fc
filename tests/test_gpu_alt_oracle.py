"""GPU: the alternate (on-the-fly) correlation lookup, output by output against
the float64 oracle.

Every kernel form of csrc/alt_corr.hip is reached through the C-ABI by a request
that can only take that form (see ``FORMS``), at every radius 0..6, at channel
counts on both sides of each switch (k-step counts 1, 2, 3, 5 and 16 of the MFMA
form's prefetch ring of 4; a divisor that is a power of two and one that is
not; one and two 256-channel slabs of the VALU form; misaligned operands), on
maps whose 4 x 8 query tiles are ragged, fewer than the 8 XCDs, no multiple of
8, and more than the 64 blocks of the ordering kernels.

Per output, with ``ref`` the float64 oracle and ``M`` the same oracle of |fmap1|,
|fmap2| (the bilinear weights are non-negative, so M is the output's weighted
sum |a||b| / sqrt(D)):

  1. where M > 0: |got - ref| <= 1e-5 M.  1e-5 is the allowance these same dot
     products have in tests/test_gpu_parity.py::test_alt_volume_gemm_against_float64;
     the arithmetic gives a few 1e-7 (the f16 pair drops lo x lo, 2^-22; f32
     accumulation over C / 16 steps; four f32 multiply-adds; one divide), and
     the oracle run in float32 stays within 1e-5 M too
     (tests/test_oracle_golden.py::test_alt_block_float32_oracle_within_the_gpu_bound);
  2. where M == 0 (window off the level, or only zero-weight taps on it) the
     output is exactly 0 — and every level of every case has outputs with M > 0;
  3. NaN exactly where the oracle has NaN (queries with a NaN / +-inf
     coordinate, on all their channels);
  4. nothing but the output is written: a guard behind it keeps its bits, and
     the levels a partial request leaves out keep the sentinel;
  5. the ordered and the tile-order MFMA forms agree bit for bit.

The ordered form picks bin order or tile order on the device; the coordinate
sets give it flows of both kinds (i.i.d. and smooth) and either choice must be
correct.  ``dxr_alt_corr_backward`` is checked the same way at the radii no
other test runs (1, 2, 5, 6).
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest
import torch

import datagen as dg
import oracle
from test_gpu_lookup_backward import poke_nonfinite

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 4096          # floats behind the output
SENTINEL = 1.5        # finite: a NaN would hide in the non-finite cases
BOUND = 1e-5          # |got - ref| <= BOUND * M


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
    return torch.from_numpy(np.array(a)).to(DEV)     # a copy: the cases' arrays are read-only


# --------------------------------------------------------------------------- cases
# (B, H, W, levels).  base: 5 x 3 = 15 query tiles of 4 x 8, ragged both ways, 15 % 8 != 0
# (the XCD remap's remainder branch), levels 18x21, 9x10, 4x5, 2x2 (windows of r >= 2 exceed
# the coarse ones, r = 6 level 1 too).  few: 6 tiles < 8 XCDs.  tpb2: 66 tiles > 64 ordering
# blocks, so two tiles per block.
SHAPES = {"base": (2, 18, 21, 4), "few": (1, 8, 20, 2), "tpb2": (1, 44, 48, 4)}

# (shape, D, r).  D = 16, 32, 48: 1-3 k steps, shorter than the prefetch ring of 4; 80: 5, a
# partial second round; 256: 16.  sqrt(D) is a power of two at 16 and 256 only.
MFMA_POINTS = ([("base", 48, r) for r in range(7)] +
               [("base", D, 4) for D in (16, 32, 80, 256)] +
               [("base", 16, 6), ("base", 80, 6), ("few", 48, 3), ("tpb2", 80, 4)])
VEC_POINTS = [("base", 36, r) for r in (0, 2, 5, 6)] + [("base", 272, 4)]
SCALAR_POINTS = [("base", 37, r) for r in (0, 2, 5, 6)]
SETS = ("uniform", "integer", "smooth")

# form -> (entry point, what makes the launcher take it)
FORMS = {
    "mfma_tile": "dxr_alt_corr_lookup: C % 16 == 0, C <= 256, 16-byte aligned operands",
    "mfma_ordered": "dxr_alt_corr_lookup_ws with dxr_alt_workspace_bytes of workspace",
    "mfma_ordered_levels2": "dxr_alt_corr_lookup_levels_ws, n_levels = 2 of 4",
    "valu_vec": "dxr_alt_corr_lookup: C % 4 == 0 and (C % 16 != 0 or C > 256)",
    "valu_scalar": "dxr_alt_corr_lookup: C % 4 != 0",
    "valu_scalar_misaligned": "dxr_alt_corr_lookup: C = 64, fmap1 4 bytes off alignment",
}


def _runs():
    runs = []
    for p in MFMA_POINTS:
        forms = ["mfma_tile", "mfma_ordered"] + (["mfma_ordered_levels2"] if p[0] != "few" else [])
        sets = SETS + (("nonfinite",) if p == ("base", 48, 4) else ())
        runs += [(f,) + p + (s,) for s in sets for f in forms]
    for p in VEC_POINTS:
        sets = SETS + (("nonfinite",) if p == ("base", 36, 2) else ())
        runs += [("valu_vec",) + p + (s,) for s in sets]
    for p in SCALAR_POINTS:
        sets = SETS + (("nonfinite",) if p == ("base", 37, 2) else ())
        runs += [("valu_scalar",) + p + (s,) for s in sets]
    runs += [("valu_scalar_misaligned", "base", 64, 3, s) for s in SETS + ("nonfinite",)]
    return runs


# the forms of one (point, set) are neighbours: the small caches below then hold what they share
RUNS = _runs()


def _seed(*key) -> int:
    """A stable seed of a case's name (no Python hash: that differs per process)."""
    s = 0
    for ch in "/".join(str(k) for k in key):
        s = (s * 131 + ord(ch)) % 1000003
    return 30000 + 16 * s


def coord_set(seed: int, name: str, B: int, H: int, W: int) -> np.ndarray:
    """[B, 2, H, W] float32.  uniform: windows all over the map, many partly off
    it; integer: zero second-tap weights; smooth: the pixel grid + a constant + a
    slow sine (neighbouring windows overlap: the flows the ordered form leaves in
    tile order); nonfinite: NaN, +-inf, 3e9 and -40 among ordinary queries."""
    if name == "uniform":
        return dg.coords(seed, B, H, W, "uniform", 8.0)
    if name == "integer":
        return dg.coords(seed, B, H, W, "integer", 4.0)
    if name == "nonfinite":
        assert B >= 2
        return poke_nonfinite(dg.coords(seed, B, H, W, "normal", 4.0))
    assert name == "smooth"
    grid = dg.coords(seed, B, H, W, "identity").astype(np.float64)
    u = 4.0 * dg.normal(seed, B * 2).reshape(B, 2, 1, 1) + 2.0 * np.sin(grid / 9.0)
    return (grid + u).astype(np.float32)


@lru_cache(maxsize=2)
def fmaps(shape: str, D: int):
    B, H, W, _ = SHAPES[shape]
    f1 = dg.fmap(_seed(shape, D, 1), B, D, H, W)
    f2 = dg.fmap(_seed(shape, D, 2), B, D, H, W)
    f1.flags.writeable = f2.flags.writeable = False
    return f1, f2


@lru_cache(maxsize=2)
def case_reference(shape: str, D: int, r: int, cset: str):
    """(coords, ref, M) of a case, read-only: the float64 oracle on the float32
    fmaps (it pools them in float32, as the block does — bit for bit, checked
    in ``operands``) and on their absolute values."""
    B, H, W, L = SHAPES[shape]
    f1, f2 = fmaps(shape, D)
    c = coord_set(_seed(shape, D, r, cset), cset, B, H, W)
    with np.errstate(invalid="ignore"):
        ref = oracle.alt_corr_block(f1, f2, c, L, r, np.float64)
        M = oracle.alt_corr_block(np.abs(f1), np.abs(f2), c, L, r, np.float64)
    for a in (c, ref, M):
        a.flags.writeable = False
    return c, ref, M


@lru_cache(maxsize=2)
def operands(shape: str, D: int):
    """The block's NHWC operands on the device (full-resolution fmap1 and the
    pooled fmap2 levels), built the way AlternateCorrBlock builds them; the
    pooled levels are the oracle's float32 pools bit for bit."""
    import dexiraft_amd
    B, H, W, L = SHAPES[shape]
    f1, f2 = fmaps(shape, D)
    ab = dexiraft_amd.AlternateCorrBlock(_t(f1), _t(f2), num_levels=L, radius=0)
    assert ab.coarse_first_level is None
    lvl = f2
    for i in range(L):
        if i:
            lvl = oracle.avg_pool2x2(lvl)
        assert np.array_equal(ab._f2_nhwc[i].cpu().numpy(), lvl.transpose(0, 2, 3, 1)), i
    return ab


def _guarded(n: int) -> torch.Tensor:
    return torch.full((n + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)


def _take(buf: torch.Tensor, shape) -> np.ndarray:
    """The output part of a guarded buffer, after checking the guard's bits."""
    torch.cuda.synchronize()
    res = buf.cpu().numpy()
    n = int(np.prod(shape))
    assert np.array_equal(res[n:].view(np.int32),
                          np.full(GUARD, SENTINEL, np.float32).view(np.int32)), \
        "the guard behind the output was written"
    return res[:n].reshape(shape)


@lru_cache(maxsize=6)
def run_form(form: str, shape: str, D: int, r: int, cset: str) -> np.ndarray:
    """One request of ``form`` into a sentinel-filled, guarded output:
    [B, L (2r+1)^2, H, W], read-only."""
    nat = _nat()
    lib = nat.load()
    B, H, W, L = SHAPES[shape]
    c, _, _ = case_reference(shape, D, r, cset)
    ab = operands(shape, D)
    K = L * (2 * r + 1) ** 2
    buf = _guarded(B * K * H * W)
    ct = _t(c)
    f1 = ab._f1_nhwc
    assert f1.data_ptr() % 16 == 0 and all(t.data_ptr() % 16 == 0 for t in ab._f2_nhwc)
    if form == "valu_scalar_misaligned":
        store = torch.empty(f1.numel() + 4, dtype=torch.float32, device=DEV)
        f1 = store[1:1 + f1.numel()].view(f1.shape)
        f1.copy_(ab._f1_nhwc)
        assert f1.data_ptr() % 16 == 4
    # each request can take one form only (launch_alt in csrc/alt_corr.hip)
    if form.startswith("mfma"):
        assert D % 16 == 0 and D <= 256
    elif form == "valu_vec":
        assert D % 4 == 0 and (D % 16 != 0 or D > 256)
    elif form == "valu_scalar":
        assert D % 4 != 0
    args = (f1.data_ptr(), ab._f2_ptrs, ct.data_ptr(), buf.data_ptr(), B, H, W, D, L)
    div = float(np.sqrt(np.float32(D), dtype=np.float32))
    s = nat.stream_of(buf)
    if form == "mfma_ordered":
        n = lib.dxr_alt_workspace_bytes(B, H, W, L)
        assert n > 0
        ws = torch.empty(n, dtype=torch.uint8, device=DEV)
        assert ws.data_ptr() % 16 == 0
        nat.check(lib.dxr_alt_corr_lookup_ws(*args, r, div, ws.data_ptr(), n, s), form)
    elif form == "mfma_ordered_levels2":
        n = lib.dxr_alt_workspace_bytes(B, H, W, 2)
        assert n > 0
        ws = torch.empty(n, dtype=torch.uint8, device=DEV)
        assert ws.data_ptr() % 16 == 0
        nat.check(lib.dxr_alt_corr_lookup_levels_ws(*args, 2, r, div, ws.data_ptr(), n, s), form)
    else:
        nat.check(lib.dxr_alt_corr_lookup(*args, r, div, s), form)
    out = _take(buf, (B, K, H, W))
    out.flags.writeable = False
    return out


# --------------------------------------------------------------------------- checks
def check_outputs(tag: str, got: np.ndarray, ref: np.ndarray, M: np.ndarray, n_groups: int) -> float:
    """Assertions 1-3 of the module's docstring on [B, n_groups * k, ...] outputs
    (a group: one level's channels); returns the largest |err| / M."""
    assert got.shape == ref.shape == M.shape and got.dtype == np.float32
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(M), nan)
    assert np.array_equal(np.isnan(got), nan), f"{tag}: NaN pattern differs from the oracle's"
    pos = M > 0
    zero = M == 0
    k = got.shape[1] // n_groups
    for lvl in range(n_groups):
        assert pos[:, lvl * k:(lvl + 1) * k].any(), f"{tag}: no output of level {lvl} has M > 0"
    err = np.abs(got[pos].astype(np.float64) - ref[pos])
    ratio = err / M[pos]
    i = int(np.argmax(ratio))
    print(f"ALT-ORACLE {tag}: max |err| / M {ratio[i]:.3e} (got {got[pos][i]:.9e} ref "
          f"{ref[pos][i]:.9e} M {M[pos][i]:.3e}), {zero.mean():.0%} exact zeros, "
          f"{int(nan.sum())} NaN")
    assert (got[zero] == 0).all(), f"{tag}: an output with no in-level tap is not exactly 0"
    assert (err <= BOUND * M[pos]).all(), f"{tag}: max |err| / M {ratio[i]:.3e} > {BOUND}"
    return float(ratio[i])


def check_nonfinite_reference(c: np.ndarray, ref: np.ndarray) -> None:
    """The oracle itself, on poke_nonfinite's queries: NaN / +-inf coordinates are
    NaN on all their channels and nothing else is; 3e9 is off every level."""
    want = np.zeros(ref.shape, dtype=bool)
    for b, y, x in ((0, 3, 5), (0, 7, 7), (0, 0, 0)):
        assert not np.isfinite(c[b, :, y, x]).all()
        want[b, :, y, x] = True
    assert np.array_equal(np.isnan(ref), want)
    assert c[0, 1, 2, 2] == np.float32(3e9) and not ref[0, :, 2, 2].any()


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    """Bit equality with NaNs in place (a NaN's payload is not compared)."""
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and
                np.array_equal(a.view(np.int32)[~na], b.view(np.int32)[~nb]))


# --------------------------------------------------------------------------- the lookup
@pytest.mark.parametrize("form,shape,D,r,cset", RUNS,
                         ids=[f"{f}-{sh}-D{D}-r{r}-{s}" for f, sh, D, r, s in RUNS])
def test_alt_lookup_matches_oracle_per_output(dx, form, shape, D, r, cset):
    B, H, W, L = SHAPES[shape]
    c, ref, M = case_reference(shape, D, r, cset)
    if cset == "nonfinite":
        check_nonfinite_reference(c, ref)
    got = run_form(form, shape, D, r, cset)
    tag = f"{form} {shape} D={D} r={r} {cset}"
    k = (2 * r + 1) ** 2
    if form == "mfma_ordered_levels2":
        # levels 2..3 are another request's: their channels keep the sentinel's bits
        rest = got[:, 2 * k:]
        assert np.array_equal(rest.view(np.int32),
                              np.full(rest.shape, SENTINEL, np.float32).view(np.int32)), \
            f"{tag}: a channel of a level that was not requested was written"
        check_outputs(tag, got[:, :2 * k], ref[:, :2 * k], M[:, :2 * k], 2)
        assert same_bits(got[:, :2 * k], run_form("mfma_tile", shape, D, r, cset)[:, :2 * k]), tag
        return
    check_outputs(tag, got, ref, M, L)
    if form == "mfma_ordered":
        assert same_bits(got, run_form("mfma_tile", shape, D, r, cset)), \
            f"{tag}: differs from the tile-order form"


# --------------------------------------------------------------------------- FFI forward
# alt_cuda_corr.forward's layouts: Nc = 2 coordinate sets per pair (the kernel's z = b * Nc + n
# with the fmaps of pair b), fmap2 of another size than fmap1, no divisor.  C = 48: the MFMA
# form in tile order, 3 k steps.
FFI = dict(B=2, H1=18, W1=21, H2=13, W2=17, C=48, Nc=2)
FFI_RUNS = [(r, s) for r in (1, 6) for s in SETS + (("nonfinite",) if r == 6 else ())]


@lru_cache(maxsize=None)
def ffi_inputs():
    B, H1, W1, H2, W2, C = (FFI[k] for k in ("B", "H1", "W1", "H2", "W2", "C"))
    f1 = dg.normal(_seed("ffi", 1), B * H1 * W1 * C).reshape(B, H1, W1, C).astype(np.float32)
    f2 = dg.normal(_seed("ffi", 2), B * H2 * W2 * C).reshape(B, H2, W2, C).astype(np.float32)
    f1.flags.writeable = f2.flags.writeable = False
    return f1, f2


@pytest.mark.parametrize("r,cset", FFI_RUNS, ids=[f"ffi_mfma_tile-r{r}-{s}" for r, s in FFI_RUNS])
def test_alt_forward_ffi_matches_oracle_per_output(dx, r, cset):
    nat = _nat()
    lib = nat.load()
    B, H1, W1, H2, W2, C, Nc = (FFI[k] for k in ("B", "H1", "W1", "H2", "W2", "C", "Nc"))
    f1, f2 = ffi_inputs()
    # the sets of all pairs as one [B * Nc, 2, H1, W1] batch, then [B, Nc, H1, W1, 2]
    c4 = coord_set(_seed("ffi", r, cset), cset, B * Nc, H1, W1)
    c = np.ascontiguousarray(c4.reshape(B, Nc, 2, H1, W1).transpose(0, 1, 3, 4, 2))
    with np.errstate(invalid="ignore"):
        ref = oracle.alt_corr_forward(f1, f2, c, r, np.float64)
        M = oracle.alt_corr_forward(np.abs(f1), np.abs(f2), c, r, np.float64)
    k = (2 * r + 1) ** 2
    shape = (B, Nc, k, H1, W1)
    assert ref.shape == shape
    if cset == "nonfinite":
        check_nonfinite_reference(c4, ref.reshape(B * Nc, k, H1, W1))
    t1, t2, ct = _t(f1), _t(f2), _t(c)
    assert t1.data_ptr() % 16 == 0 and t2.data_ptr() % 16 == 0
    buf = _guarded(int(np.prod(shape)))
    nat.check(lib.dxr_alt_corr_forward(t1.data_ptr(), t2.data_ptr(), ct.data_ptr(), buf.data_ptr(),
                                       B, H1, W1, H2, W2, C, Nc, r, nat.stream_of(buf)), "ffi")
    got = _take(buf, shape)
    # one group per coordinate set: each must have live outputs
    check_outputs(f"ffi_mfma_tile r={r} {cset}", got.reshape(B, Nc * k, H1, W1),
                  ref.reshape(B, Nc * k, H1, W1), M.reshape(B, Nc * k, H1, W1), Nc)


# --------------------------------------------------------------------------- backward
BW = dict(B=2, H1=9, W1=13, H2=7, W2=11, Nc=2)


def _bw_inputs(C: int, r: int):
    B, H1, W1, H2, W2, N = (BW[k] for k in ("B", "H1", "W1", "H2", "W2", "Nc"))
    rd = 2 * r + 1
    sd = _seed("bw", C, r)
    f1 = dg.normal(sd, B * H1 * W1 * C).reshape(B, H1, W1, C).astype(np.float32)
    f2 = dg.normal(sd + 1, B * H2 * W2 * C).reshape(B, H2, W2, C).astype(np.float32)
    # x in [-4, 5), y in [-3, 13): windows off every side of the 7 x 11 map, and at
    # r <= 2 columns on the right that no window reaches
    u = dg.uniform(sd + 2, B * N * H1 * W1 * 2).reshape(B, N, H1, W1, 2)
    c = (u * np.array([9.0, 16.0]) - np.array([4.0, 3.0])).astype(np.float32)
    g = dg.normal(sd + 3, B * N * rd * rd * H1 * W1).reshape(B, N, rd * rd, H1, W1)
    return f1, f2, c, g.astype(np.float32)


def _contributions(c: np.ndarray, r: int, H2: int, W2: int) -> np.ndarray:
    """[B, H2, W2]: how many (coordinate set, query, window cell) triples land on
    each fmap2 cell — the oracle's (and the kernel's) indices
    floor(coordinate) - r + i, i in [0, 2r + 1]."""
    B = c.shape[0]
    x0 = np.floor(c[..., 0]).astype(np.int64).reshape(B, -1)
    y0 = np.floor(c[..., 1]).astype(np.int64).reshape(B, -1)
    count = np.zeros((B, H2, W2), dtype=np.int64)
    for iy in range(2 * r + 2):
        for ix in range(2 * r + 2):
            h2, w2 = y0 - r + iy, x0 - r + ix
            ok = (h2 >= 0) & (h2 < H2) & (w2 >= 0) & (w2 < W2)
            for b in range(B):
                np.add.at(count[b], (h2[b][ok[b]], w2[b][ok[b]]), 1)
    return count


@pytest.mark.parametrize("C", [20, 300])
@pytest.mark.parametrize("r", [1, 2, 5, 6])
def test_alt_backward_matches_oracle_per_element(dx, C, r):
    """alt_cuda_corr.backward at the radii no other test runs (r = 5 and 6: two
    and three lane groups of window weights), C within one 256-channel slab and
    across two, against oracle.alt_corr_backward in float64 with M the same
    oracle of |fmap1|, |fmap2|, |corr_grad|.

    fmap1_grad is summed in a fixed order by the query's own wave: 1e-5 M, as
    the forward.  fmap2_grad is summed by atomics in arbitrary order: a sum of
    n float32 terms in any order is within (n - 1) 2^-24 of sum |terms|, and
    each term (a weight of three products and up to four adds, times fmap1)
    carries a few 2^-24 of its own; with n the largest number of contributions
    to one cell at these inputs (counted from the window indices) the allowance
    is 4 n 2^-24 M.  A cell no window reaches is exactly 0 and coords_grad is
    all zeros."""
    H2, W2 = BW["H2"], BW["W2"]
    f1, f2, c, g = _bw_inputs(C, r)
    r1, r2, _ = oracle.alt_corr_backward(f1, f2, c, g, r)
    m1, m2, _ = oracle.alt_corr_backward(np.abs(f1), np.abs(f2), c, np.abs(g), r)
    count = _contributions(c, r, H2, W2)
    n = int(count.max())
    assert n > 1 and (m1 > 0).any()
    if r <= 2:      # small windows: queries wholly off the map, and cells no window reaches
        assert (m1 == 0).any() and (count == 0).any()
    g1, g2, gc = dx.alt_cuda_corr.backward(_t(f1), _t(f2), _t(c), _t(g), r)
    torch.cuda.synchronize()
    g1, g2 = g1.cpu().numpy(), g2.cpu().numpy()
    assert tuple(gc.shape) == c.shape and not gc.any()
    assert np.isfinite(g1).all() and np.isfinite(g2).all()
    e1 = np.abs(g1.astype(np.float64) - r1)
    e2 = np.abs(g2.astype(np.float64) - r2)
    allow2 = 4.0 * n * 2.0 ** -24
    with np.errstate(divide="ignore", invalid="ignore"):
        q1 = np.where(m1 > 0, e1 / m1, 0.0).max()
        q2 = np.where(m2 > 0, e2 / m2, 0.0).max()
    print(f"ALT-ORACLE backward C={C} r={r}: fmap1_grad max |err| / M {q1:.3e} (bound {BOUND}), "
          f"fmap2_grad {q2:.3e} (bound {allow2:.3e}, at most {n} contributions per cell)")
    assert not g2[count == 0].any(), "a fmap2_grad cell no window reaches is not exactly 0"
    assert (e1 <= BOUND * m1).all()
    assert (e2 <= allow2 * m2).all()
