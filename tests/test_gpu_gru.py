"""GPU: the fused SepConvGRU forward (include/dexiraft_gru.h, csrc/gru_sepconv.hip)
against the float64 oracle tests/gru_oracle.py, stage by stage, and its exact
properties.

Stage contracts.  Each stage is checked on its own inputs, read back from the
workspace the kernels wrote, so no rounding flip of one stage shows in the next.
u = 2^-24.  A pre-activation is b + 5 (Ch + Cx) products; the kernel sums them as
5 (Ch + Cx) / 16 MFMA steps of 16 products each on one float32 accumulator and
adds the bias last, so its longest accumulation chain is
n = 5 (Ch + Cx) / 16 + 16 (the steps, the 16 products inside one step, the bias
included), and with S = |b| + sum |Wc| |a| its error is at most E = n u S:
  |z - sigmoid(P64)|   <= E / 4 + 8u
  |widen(rh) - r64 h|  <= |h| (E / 4 + 8u) + 2^-p |r64 h| + 1e-37   (p = 11 / 8)
  |h' - h'64|          <= (|h| + |q64|) (E_z / 4 + 8u) + |z64| (E_q + 8u)
                          + 4u (|h| + |q64|)
with one further rne_c (2^-p |h'64|) for a 16-bit output of the vertical QH.
8u covers the evaluation of sigmoid / tanh and the product, 4u the blend.  Every
test prints the largest fraction of its bound that was used.

Inputs.  The rh bound's rounding term is relative (2^-p |r64 h|), which holds for
rne_c only inside c's normal range: below 2^-14 float16's spacing is 2^-24 whatever
the value, so rne_c itself errs by up to 2^-25 there.  The stage tests therefore
run both axes on states with |h| >= 1/16 (gru_oracle.case, h_floor; r stays above
0.009, so |r h| >= 1e-3 >> 2^-14), which test_stage_zr asserts from the oracle's
products before it looks at the kernel's; the horizontal and the vertical pair of
stages each start from the packed inputs, so the vertical stage's state is chosen
and not whatever the horizontal one left.  float16's subnormal range has a test of
its own, test_rh_below_float16_normal_range, with the format's floor in the bound;
bfloat16's normal range reaches down to 2^-126, so there the bounds as they stand
are also checked on an unrestricted tanh(N(0, 1)) state
(test_stages_on_an_unrestricted_state_bfloat16).
The five launches in sequence are covered by the exact tests and the goldens.

Tiles.  A gate launch runs 32-pixel workgroups while it has at most 768 of them and
64-pixel ones beyond (launch_gate in csrc/gru_sepconv.hip).  (4, 65, 70) has
4 x 65 x 3 = 780 tiles along W and 4 x 70 x 3 = 840 along H, so all four gate
launches take the 64-pixel form; a row ends inside its second segment
(70 = 64 + 6), whose second 32-pixel block lies wholly past the row's end, and so
does a column (65 = 64 + 1).  One image of it alone has 195 / 210 tiles and takes
the 32-pixel form, so
test_64_pixel_tiles_equal_32_pixel_tiles compares the two forms bit for bit.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest
import torch

import gru_oracle as go
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
CNAME = {torch.float16: "f16", torch.bfloat16: "bf16"}
DTYPES = [torch.float16, torch.bfloat16]
# (N, H, W, Ch, Cx): every tap padded; rows and columns shorter than the halo; segments
# that end inside a row (67 = 2 x 32 + 3, 130 = 4 x 32 + 2); a second image directly after
# the first; the production channels with a full K loop, the source switch at channel
# 128 and one segment boundary; and, last, the 64-pixel tiles on both axes (module docstring)
CASES = [(1, 1, 1, 16, 32), (1, 1, 5, 16, 32), (2, 3, 1, 16, 32), (2, 5, 67, 16, 32),
         (1, 9, 130, 16, 32), (1, 3, 70, 128, 256), (4, 65, 70, 16, 32)]
TILE64_ABOVE = 768      # launch_gate: 64-pixel workgroups above this many 32-pixel tiles
IDS = [f"{n}x{h}x{w}_c{ch}" for n, h, w, ch, _ in CASES]


def dev():
    assert torch.cuda.is_available(), "needs a HIP device"
    return torch.device("cuda", 0)


def nchw64(t: torch.Tensor) -> np.ndarray:
    """A channels-last workspace view [N, H, W, C] as float64 NCHW on the host."""
    return t.permute(0, 3, 1, 2).double().cpu().numpy()


class Stages:
    """The dxg_ entry points on torch tensors, weights packed once per axis."""

    def __init__(self, weights: dict, c: torch.dtype):
        from dexiraft_amd import _native, gru
        self.nat, self.lib, self.views = _native, _native.load_gru(), gru.workspace_views
        self.c, self.cflag = c, gru._DXG[c]
        self.dxg = gru._DXG
        w = weights["convz1.weight"]
        self.ch, self.cx = w.shape[0], w.shape[1] - w.shape[0]
        nbytes = self.lib.dxg_sepconv_packed_weight_bytes(self.ch, self.cx)
        self.packed = []
        for axis in range(2):
            t = [torch.from_numpy(np.ascontiguousarray(weights[f"{n}.{k}"])).to(dev())
                 for n in go.NAMES[3 * axis:3 * axis + 3] for k in ("weight", "bias")]
            buf = torch.empty(nbytes, dtype=torch.uint8, device=dev())
            self.check(self.lib.dxg_sepconv_pack_weights(
                t[0].data_ptr(), t[2].data_ptr(), t[4].data_ptr(), t[1].data_ptr(), t[3].data_ptr(),
                t[5].data_ptr(), self.ch, self.cx, self.cflag, buf.data_ptr(), nbytes,
                self.stream()))
            self.packed.append(buf)
        torch.cuda.synchronize()

    def stream(self):
        return torch.cuda.current_stream(dev()).cuda_stream

    def check(self, status):
        self.nat.check(status, "dxg")

    def workspace(self, N, H, W):
        nbytes = self.lib.dxg_sepconv_workspace_bytes(N, H, W, self.ch, self.cx)
        ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev())
        return ws, self.views(ws, N, H, W, self.ch, self.cx, self.c)

    def geo(self, h):
        return (h.shape[0], h.shape[2], h.shape[3], self.ch, self.cx)

    def pack_inputs(self, h, x, ws):
        self.check(self.lib.dxg_sepconv_pack_inputs(
            h.data_ptr(), self.dxg[h.dtype], x.data_ptr(), self.dxg[x.dtype], *self.geo(h),
            self.cflag, ws.data_ptr(), ws.numel(), self.stream()))

    def zr(self, axis, h, ws):
        self.check(self.lib.dxg_sepconv_gate_zr(self.packed[axis].data_ptr(), axis, *self.geo(h),
                                                self.cflag, ws.data_ptr(), ws.numel(), self.stream()))

    def qh(self, axis, h, ws, out=None):
        self.check(self.lib.dxg_sepconv_gate_qh(
            self.packed[axis].data_ptr(), axis, *self.geo(h), self.cflag,
            None if out is None else out.data_ptr(), 0 if out is None else self.dxg[out.dtype],
            ws.data_ptr(), ws.numel(), self.stream()))

    def gru(self, h, x, out_dtype=None):
        ws, _ = self.workspace(h.shape[0], h.shape[2], h.shape[3])
        out = torch.empty(h.shape, dtype=out_dtype or h.dtype, device=h.device)
        self.check(self.lib.dxg_sepconv_gru(
            h.data_ptr(), self.dxg[h.dtype], x.data_ptr(), self.dxg[x.dtype],
            self.packed[0].data_ptr(), self.packed[1].data_ptr(), *self.geo(h), self.cflag,
            out.data_ptr(), self.dxg[out.dtype], ws.data_ptr(), ws.numel(), self.stream()))
        return out


H_FLOOR = 1.0 / 16
NORMAL_MIN = {"f16": 2.0 ** -14, "bf16": 2.0 ** -126}   # the smallest normal number of c


def tiles32(N, H, W, axis):
    """32-pixel tiles of a gate launch along W (axis 0) or H (axis 1), as launch_gate counts."""
    lines, L = (H, W) if axis == 0 else (W, H)
    return N * lines * ((L + 31) // 32)


@lru_cache(maxsize=None)
def record(case: int, c: torch.dtype, h_floor: float = H_FLOOR) -> dict:
    """One case: per axis, pack -> ZR -> QH from the packed inputs with a snapshot of
    the workspace after every launch (host float64 NCHW); the five launches in
    sequence; and the oracle's operands.  Shared by the tests; read only."""
    N, H, W, Ch, Cx = CASES[case]
    h, x, weights = go.case(9000 + 100 * case, N, H, W, Ch, Cx, h_floor=h_floor)
    st = Stages(weights, c)
    ht, xt = torch.from_numpy(h).to(dev()), torch.from_numpy(x).to(dev())
    snaps = {}
    out_v = torch.empty_like(ht)
    out16_v = torch.empty_like(ht, dtype=c)
    for axis in range(2):
        ws, v = st.workspace(N, H, W)

        def snap(name):
            torch.cuda.synchronize()
            snaps[name] = {k: nchw64(t) for k, t in v.items()}

        st.pack_inputs(ht, xt, ws)
        torch.cuda.synchronize()
        if axis == 0:
            packed_views = {k: t.clone() for k, t in v.items()}
        snap(f"in{axis}")
        st.zr(axis, ht, ws)
        snap(f"zr{axis}")
        if axis == 0:
            st.qh(0, ht, ws)
        else:
            st.qh(1, ht, ws, out_v)
            st.qh(1, ht, ws, out16_v)
        snap(f"qh{axis}")
    # the five launches in sequence
    ws, _ = st.workspace(N, H, W)
    out = torch.empty_like(ht)
    st.pack_inputs(ht, xt, ws)
    st.zr(0, ht, ws)
    st.qh(0, ht, ws)
    st.zr(1, ht, ws)
    st.qh(1, ht, ws, out)
    torch.cuda.synchronize()
    cn = CNAME[c]
    wc = {n: go.rne(go.w3(weights[f"{n}.weight"]), cn) for n in go.NAMES}
    b = {n: weights[f"{n}.bias"].astype(np.float64) for n in go.NAMES}
    return {"st": st, "h": ht, "x": xt, "weights": weights, "snaps": snaps, "out": out,
            "out_v": out_v, "out16_v": out16_v, "packed_views": packed_views, "wc": wc, "b": b,
            "cn": cn, "n": 5 * (Ch + Cx) // 16 + 16}


def used(err, bound, what):
    frac = float((err / bound).max())
    print(f"{what}: largest fraction of the bound used {frac:.3f}")
    assert np.isfinite(err).all() and frac <= 1.0, (what, frac)


@pytest.mark.parametrize("c", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_pack_inputs_is_a_cast_and_a_permute(case, c):
    r = record(case, c)
    v = r["packed_views"]
    assert torch.equal(v["h32"], r["h"].permute(0, 2, 3, 1))
    assert torch.equal(v["hc"], r["h"].to(c).permute(0, 2, 3, 1))
    assert torch.equal(v["xc"], r["x"].to(c).permute(0, 2, 3, 1))
    # 16-bit sources of either kind, read in place
    st = r["st"]
    for dt in DTYPES:
        h16, x16 = r["h"].to(dt), r["x"].to(dt)
        N, _, H, W = r["h"].shape
        ws, w = st.workspace(N, H, W)
        st.pack_inputs(h16, x16, ws)
        torch.cuda.synchronize()
        assert torch.equal(w["h32"], h16.float().permute(0, 2, 3, 1))
        assert torch.equal(w["hc"], h16.float().to(c).permute(0, 2, 3, 1))
        assert torch.equal(w["xc"], x16.float().to(c).permute(0, 2, 3, 1))


@pytest.mark.parametrize("axis", [0, 1], ids=["horizontal", "vertical"])
@pytest.mark.parametrize("c", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_stage_zr(case, c, axis):
    """z and rh against the oracle on the stage's own inputs."""
    check_stage_zr(record(case, c), axis)


def check_stage_zr(r, axis):
    before = r["snaps"][f"in{axis}"]
    after = r["snaps"][f"zr{axis}"]
    nz, nr = go.NAMES[3 * axis], go.NAMES[3 * axis + 1]
    h = before["h32"]
    o = go.stage_zr(before["hc"], before["xc"], h, r["wc"][nz], r["b"][nz], r["wc"][nr], r["b"][nr],
                    axis, r["cn"])
    n, p = r["n"], go.P_BITS[r["cn"]]
    # the inputs keep every product inside c's normal range (module docstring)
    assert np.abs(o["rh_exact"]).min() >= NORMAL_MIN[r["cn"]], np.abs(o["rh_exact"]).min()
    used(np.abs(after["z"] - o["z"]), n * U * o["Sz"] / 4 + 8 * U, "z")
    bound = np.abs(h) * (n * U * o["Sr"] / 4 + 8 * U) + 2.0 ** -p * np.abs(o["rh_exact"]) + 1e-37
    used(np.abs(after["rh"] - o["rh_exact"]), bound, "rh")
    for k in ("h32", "hc", "xc"):                       # its inputs are left as they were
        assert np.array_equal(after[k], before[k])


@pytest.mark.parametrize("axis", [0, 1], ids=["horizontal", "vertical"])
def test_rh_below_float16_normal_range(axis):
    """c = float16 and a state scaled by 2^-13, so that every product |r h| is below
    2^-13 and most are subnormal in float16.  There rne_c's error is half the
    subnormal spacing, 2^-25, whatever the value, so the rounding term of the rh
    bound is max(2^-11 |r64 h|, 2^-25); the rest of the bound is test_stage_zr's.
    z does not depend on the scale of h's rounding and keeps its bound."""
    case, c = 3, torch.float16
    N, H, W, Ch, Cx = CASES[case]
    h, x, weights = go.case(9000 + 100 * case, N, H, W, Ch, Cx, h_floor=H_FLOOR)
    h = (h * np.float32(2.0 ** -13)).astype(np.float32)
    st = Stages(weights, c)
    ht, xt = torch.from_numpy(h).to(dev()), torch.from_numpy(x).to(dev())
    ws, v = st.workspace(N, H, W)
    st.pack_inputs(ht, xt, ws)
    torch.cuda.synchronize()
    before = {k: nchw64(t) for k, t in v.items()}
    st.zr(axis, ht, ws)
    torch.cuda.synchronize()
    after = {k: nchw64(t) for k, t in v.items()}
    nz, nr = go.NAMES[3 * axis], go.NAMES[3 * axis + 1]
    wz, wr = (go.rne(go.w3(weights[f"{k}.weight"]), "f16") for k in (nz, nr))
    bz, br = (weights[f"{k}.bias"].astype(np.float64) for k in (nz, nr))
    h64 = before["h32"]
    assert np.array_equal(h64, h.astype(np.float64))
    o = go.stage_zr(before["hc"], before["xc"], h64, wz, bz, wr, br, axis, "f16")
    sub = np.abs(o["rh_exact"]) < 2.0 ** -14
    print(f"{int(sub.sum())} of {sub.size} products are subnormal in float16")
    assert sub.mean() > 0.5 and np.abs(o["rh_exact"]).max() < 2.0 ** -13
    n = 5 * (Ch + Cx) // 16 + 16
    used(np.abs(after["z"] - o["z"]), n * U * o["Sz"] / 4 + 8 * U, "z")
    bound = np.abs(h64) * (n * U * o["Sr"] / 4 + 8 * U) \
        + np.maximum(2.0 ** -11 * np.abs(o["rh_exact"]), 2.0 ** -25)
    used(np.abs(after["rh"] - o["rh_exact"]), bound, "rh (float16 subnormal range)")


@pytest.mark.parametrize("axis", [0, 1], ids=["horizontal", "vertical"])
@pytest.mark.parametrize("c", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_stage_qh(case, c, axis):
    check_stage_qh(record(case, c), axis)


def check_stage_qh(r, axis):
    c = r["st"].c
    zr_in = r["snaps"][f"in{axis}"]
    before = r["snaps"][f"zr{axis}"]
    nz, nr, nq = go.NAMES[3 * axis:3 * axis + 3]
    h = before["h32"]
    # z64 from the ZR stage's own inputs, q64 from the rh the kernel wrote
    ozr = go.stage_zr(zr_in["hc"], zr_in["xc"], h, r["wc"][nz], r["b"][nz], r["wc"][nr], r["b"][nr],
                      axis, r["cn"])
    o = go.stage_qh(before["rh"], before["xc"], ozr["z"], h, r["wc"][nq], r["b"][nq], axis)
    n, p = r["n"], go.P_BITS[r["cn"]]
    hq = np.abs(h) + np.abs(o["q"])
    bound = hq * (n * U * ozr["Sz"] / 4 + 8 * U) + np.abs(ozr["z"]) * (n * U * o["Sq"] + 8 * U) \
        + 4 * U * hq
    if axis == 0:
        after = r["snaps"]["qh0"]
        used(np.abs(after["h32"] - o["h"]), bound, "h' (state)")
        assert np.array_equal(after["hc"], go.rne(after["h32"], r["cn"]))   # hc = rne_c(h32)
        for k in ("xc", "z", "rh"):
            assert np.array_equal(after[k], before[k])
    else:
        out = r["out_v"].double().cpu().numpy()
        used(np.abs(out - o["h"]), bound, "h' (float32 output)")
        out16 = r["out16_v"].double().cpu().numpy()
        used(np.abs(out16 - o["h"]), bound + 2.0 ** -p * np.abs(o["h"]), "h' (16-bit output)")
        assert torch.equal(r["out16_v"], r["out_v"].to(c))                  # rounded once
        for k in ("h32", "hc", "xc", "z", "rh"):
            assert np.array_equal(r["snaps"]["qh1"][k], before[k])


@pytest.mark.parametrize("axis", [0, 1], ids=["horizontal", "vertical"])
def test_stages_on_an_unrestricted_state_bfloat16(axis):
    """c = bfloat16 and h = tanh(N(0, 1)) as it comes, small values included: bfloat16
    has float32's exponent range, so rne_c is within 2^-8 relative of every product
    here (asserted from the oracle's products) and the stage bounds hold as stated."""
    r = record(3, torch.bfloat16, 0.0)
    assert np.abs(r["h"].cpu().numpy()).min() < H_FLOOR / 64      # the state is not floored
    check_stage_zr(r, axis)
    check_stage_qh(r, axis)


@pytest.mark.parametrize("c", DTYPES, ids=["f16", "bf16"])
def test_64_pixel_tiles_equal_32_pixel_tiles(c):
    """The batch-4 call of (4, 65, 70) runs every gate launch in 64-pixel tiles, the
    four batch-1 calls in 32-pixel tiles (asserted from launch_gate's rule): the state
    after the horizontal pair, z and rh of the vertical pair, the packed operands and
    the output are equal bit for bit, so the tile changes no value."""
    case = len(CASES) - 1
    N, H, W, Ch, Cx = CASES[case]
    for axis in range(2):
        assert tiles32(N, H, W, axis) > TILE64_ABOVE >= tiles32(1, H, W, axis)
        assert (H if axis else W) > 32
    r = record(case, c)
    st, h, x = r["st"], r["h"], r["x"]

    def run(hh, xx):
        ws, v = st.workspace(hh.shape[0], H, W)
        out = torch.empty_like(hh)
        st.pack_inputs(hh, xx, ws)
        for axis in range(2):
            st.zr(axis, hh, ws)
            st.qh(axis, hh, ws, out if axis else None)
        torch.cuda.synchronize()
        return v, out

    v4, out4 = run(h, x)
    assert torch.equal(out4, r["out"])
    for i in range(N):
        v1, out1 = run(h[i:i + 1].contiguous(), x[i:i + 1].contiguous())
        assert torch.equal(out1, out4[i:i + 1])
        for k in ("h32", "hc", "xc", "z", "rh"):
            assert torch.equal(v1[k], v4[k][i:i + 1]), (i, k)


@pytest.mark.parametrize("c", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_gru_equals_the_stages_composed_and_itself(case, c):
    import dexiraft_amd as dx
    r = record(case, c)
    st, h, x = r["st"], r["h"], r["x"]
    out = st.gru(h, x)
    assert torch.equal(out, r["out"])                   # dxg_sepconv_gru == the five stage calls
    assert torch.equal(st.gru(h, x), out)               # two runs
    mod = dx.SepConvGRU({k: torch.from_numpy(v) for k, v in r["weights"].items()}, compute_dtype=c)
    with torch.no_grad():
        got = mod(h, x)
    assert got.dtype == h.dtype and torch.equal(got, out)
    if h.shape[0] > 1:                                  # a batch-N call is N batch-1 calls
        for i in range(h.shape[0]):
            assert torch.equal(st.gru(h[i:i + 1].contiguous(), x[i:i + 1].contiguous()),
                               out[i:i + 1])
    for dt in DTYPES:                                   # 16-bit inputs == their widened values
        h16, x16 = h.to(dt), x.to(dt)
        with torch.no_grad():
            o16 = mod(h16, x16)
        assert o16.dtype == dt
        assert torch.equal(o16, st.gru(h16.float(), x16.float()).to(dt))
        assert torch.equal(mod(h16, x), st.gru(h16.float(), x).to(dt))


@pytest.mark.parametrize("c", DTYPES, ids=["f16", "bf16"])
def test_graph_replay_equals_eager(c):
    import dexiraft_amd as dx
    r = record(3, c)
    mod = dx.SepConvGRU({k: torch.from_numpy(v) for k, v in r["weights"].items()}, compute_dtype=c)
    h, x = r["h"].clone(), r["x"].clone()
    stream = torch.cuda.Stream(device=dev())
    stream.wait_stream(torch.cuda.current_stream(dev()))
    with torch.no_grad(), torch.cuda.stream(stream):
        eager = mod(h, x)                               # packs the weights outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            out = mod(h, x)
        out.zero_()
        graph.replay()
        stream.synchronize()
        assert torch.equal(out, eager) and torch.equal(eager, r["out"])
        h.copy_(r["h"].flip(0))                         # new inputs through the same graph
        x.copy_(r["x"].flip(0))
        graph.replay()
        stream.synchronize()
        assert torch.equal(out, r["out"].flip(0))
    torch.cuda.current_stream(dev()).wait_stream(stream)


@pytest.mark.parametrize("c", DTYPES, ids=["f16", "bf16"])
def test_horizontal_taps_past_the_row_ends_read_exact_zeros(c):
    """Rows 0 and 2 of both images hold very large finite values in columns 0 and
    W - 1, row 1 and everything else is zero, and the centre-tap weights are zero.
    Then every pre-activation of row 1, and of rows 0 and 2 in columns 0, W - 1 and
    3 .. W - 4, is its bias alone: those outputs must equal, bit for bit, a run on
    all-zero inputs.  A tap that read the neighbouring row, the next image or
    anything but zero past a row's end would bring a large value in."""
    N, H, W, Ch, Cx = 2, 3, 9, 16, 32
    _, _, weights = go.case(9900, N, H, W, Ch, Cx)
    for n in go.NAMES[:3]:
        weights[f"{n}.weight"][:, :, 0, 2] = 0.0
    st = Stages(weights, c)
    big = 6.0e4 if c == torch.float16 else 1.0e38
    sign = torch.tensor([1.0, -1.0], device=dev()).repeat(24)
    runs = []
    for poison in (False, True):
        h = torch.zeros(N, Ch, H, W, device=dev())
        x = torch.zeros(N, Cx, H, W, device=dev())
        if poison:
            for row in (0, 2):
                for col in (0, W - 1):
                    h[:, :, row, col] = big * sign[:Ch]
                    x[:, :, row, col] = -big * sign[:Cx]
        ws, v = st.workspace(N, H, W)
        st.pack_inputs(h, x, ws)
        st.zr(0, h, ws)
        torch.cuda.synchronize()
        z, rh = v["z"].clone(), v["rh"].clone()
        st.qh(0, h, ws)
        torch.cuda.synchronize()
        runs.append((z, rh, v["h32"].clone(), v["hc"].clone()))
    (z0, rh0, h0, hc0), (z1, rh1, h1, hc1) = runs
    assert torch.isfinite(z0).all() and (z0 > 0).all() and (h0 != 0).any()
    cols = [0, W - 1] + list(range(3, W - 3))
    for a, b in ((z0, z1), (rh0, rh1), (h0, h1), (hc0, hc1)):
        assert torch.equal(a[:, 1], b[:, 1])                              # the middle row
    assert torch.equal(z0[:, :, cols], z1[:, :, cols])                    # the poisoned rows
    assert not torch.equal(z0[:, 0, 1], z1[:, 0, 1])                      # the poison is seen


@pytest.mark.parametrize("c", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("name", ["gru_c16_b2", "gru_c32"])
def test_end_to_end_against_the_reference(name, c):
    """d = max |oracle with the roundings - golden| is the cost of the 16-bit
    operands alone (computed on the host, no code under test); the module stays
    within 2 d of the reference's float32 output.  The factor of two covers rh / hc
    values that round the other way when a float32 sum lands within E of a rounding
    boundary, an effect of the order of the operand rounding itself."""
    import dexiraft_amd as dx
    with np.load(GOLDEN / f"{name}.npz") as z:
        seed, N, H, W, Ch, Cx = (int(v) for v in z["case"])
        golden = z["out"].astype(np.float64)
    h, x, weights = go.case(seed, N, H, W, Ch, Cx)
    d = float(np.abs(go.forward(h, x, weights, CNAME[c]) - golden).max())
    mod = dx.SepConvGRU({k: torch.from_numpy(v) for k, v in weights.items()}, compute_dtype=c)
    with torch.no_grad():
        out = mod(torch.from_numpy(h).to(dev()), torch.from_numpy(x).to(dev()))
    err = float(np.abs(out.double().cpu().numpy() - golden).max())
    print(f"{name} {CNAME[c]}: d = {d:.3e}, module vs golden {err:.3e} ({err / d:.2f} d)")
    assert out.dtype == torch.float32 and np.isfinite(err) and err <= 2 * d
