"""GPU: every pyramid build kernel, cell by cell against float64.

Each request of tests/build_oracle.py's ``REQUESTS`` reaches one row of the
planner's table (tests/test_build_plan.py asks the planner which, on a CPU, at
these shapes and alignments) and goes through the C ABI as
test_build_kernel_by_request sends its own; the whole pyramid comes back through
``dxr_pyramid_unpack`` and every cell of every level is held to the bound of its
kernel's arithmetic and cell type (build_oracle's module docstring derives them
from what the kernels document; nothing in them is measured).  Cells whose
products are all zero must be exactly zero, everything is finite (float16 cells
beyond the format's range are the infinity of their sign), and the pyramid buffer
is NaN before the build, so a cell nobody wrote shows.  Both data kinds run:
``uniform`` (the N(1.1, 1.45^2) fmaps of the max-norm tests) and ``wide`` (pixel
magnitudes over 2^+-12, channels over 2^-18..1 inside a pixel, zeros and dead
pixels).  tests/test_build_bound_cpu.py shows on the host what that buys: an
arithmetic that loses a cross product, the low parts, the per-pixel scale, the
float32 pooling, the floor mode or a page's target column exceeds these bounds
where test_build_kernel_by_request's tolerance lets it through.

Every test prints the largest fraction of the bound used per level.

Measured on an MI355X (largest |err| / bound at levels 0 / 1 / 2 / 3; 16-bit cells use their
half unit in the last place to the full, as any correct rounding does):

  request                   uniform                         wide
  dma-nchw                  0.094 / 0.049 / 0.054 / 0.025   0.237 / 0.162 / 0.129 / 0.081
  dma-nchw-d256             0.079 / 0.042 / 0.020 / 0.014   0.148 / 0.141 / 0.108 / 0.041
  dma-nchw-odd              0.104 / 0.056 / 0.038 / 0.025   0.271 / 0.229 / 0.173 / 0.090
  dma-nchw-two              0.107 / 0.053 / 0.038 / 0.034   0.278 / 0.224 / 0.197 / 0.090
  dma-nchw-whole            0.145 / 0.078 / 0.051 / 0.039   0.305 / 0.253 / 0.219 / 0.127
  dma-nchw-bf16cells        0.999 / 0.999 / 0.999 / 0.996   0.999 / 0.999 / 0.997 / 0.997
  dma-nchw-f16cells         0.994 / 0.991 / 0.989 / 0.987   1.000 / 0.996 / 0.991 / 0.987
  dma-nhwc                  0.094 / 0.049 / 0.054 / 0.025   0.237 / 0.162 / 0.129 / 0.081
  dma-nhwc-odd              0.104 / 0.056 / 0.038 / 0.025   0.271 / 0.229 / 0.173 / 0.090
  dma-nhwc-f16cells         0.994 / 0.991 / 0.989 / 0.987   1.000 / 0.996 / 0.991 / 0.987
  split-f4                  0.105 / 0.062 / 0.061 / 0.029   0.603 / 0.408 / 0.147 / 0.077
  split-f4-two              0.096 / 0.058 / 0.045 / 0.034   0.435 / 0.302 / 0.167 / 0.089
  split-f4-bf16cells        0.999 / 0.999 / 0.999 / 0.996   0.999 / 0.999 / 0.997 / 0.997
  split-f2                  0.104 / 0.055 / 0.038 / 0.035   0.478 / 0.349 / 0.166 / 0.107
  split-nhwc                0.105 / 0.062 / 0.061 / 0.029   0.603 / 0.408 / 0.147 / 0.077
  split-nhwc-even           0.104 / 0.055 / 0.038 / 0.035   0.478 / 0.349 / 0.166 / 0.107
  exact-vec                 0.210 / 0.101 / 0.057 / 0.035   0.346 / 0.321 / 0.166 / 0.086
  exact-vec-d24             0.226 / 0.097 / 0.069 / 0.068   0.412 / 0.306 / 0.258 / 0.128
  exact-vec-bf16cells       0.999 / 0.999 / 0.999 / 0.996   0.999 / 0.999 / 0.997 / 0.998
  exact-scalar-d24          0.250 / 0.100 / 0.056 / 0.051   0.338 / 0.243 / 0.179 / 0.090
  pack-dma16-bf16           0.999 / 0.999 / 0.999 / 0.998   0.999 / 0.999 / 0.999 / 0.992
  pack-dma16-bf16-f32cells  0.113 / 0.058 / 0.043 / 0.030   0.208 / 0.205 / 0.124 / 0.049
  pack-dma16-bf16-odd       0.999 / 0.999 / 0.998 / 0.988   0.999 / 0.999 / 0.997 / 0.998
  pack-dma16-bf16-two       0.999 / 0.999 / 0.998 / 0.998   0.999 / 0.999 / 0.999 / 0.998
  pack-dma16-bf16-whole     0.161 / 0.089 / 0.053 / 0.042   0.303 / 0.238 / 0.196 / 0.160
  pack-dma16-f16            0.112 / 0.066 / 0.049 / 0.033   0.228 / 0.171 / 0.140 / 0.054
  pack-dma16-f16-f16cells   0.995 / 0.992 / 0.994 / 0.987   1.000 / 0.997 / 0.987 / 0.976
  dma16-nhwc-bf16           0.999 / 0.999 / 0.999 / 0.998   0.999 / 0.999 / 0.999 / 0.992
  dma16-nhwc-bf16-f32cells  0.113 / 0.058 / 0.043 / 0.030   0.208 / 0.205 / 0.124 / 0.049
  dma16-nhwc-f16            0.137 / 0.065 / 0.040 / 0.030   0.199 / 0.176 / 0.141 / 0.083
  dma16-nhwc-f16-f16cells   0.995 / 0.992 / 0.994 / 0.987   1.000 / 0.997 / 0.987 / 0.976
  bf16-q2                   0.999 / 0.999 / 0.999 / 0.998   0.999 / 0.999 / 0.999 / 0.992
  bf16-q2-f32cells          0.113 / 0.058 / 0.043 / 0.030   0.208 / 0.205 / 0.124 / 0.049
  bf16-q2-d48               1.000 / 0.999 / 0.999 / 0.994   0.999 / 0.999 / 0.999 / 0.997
  bf16-scalar               0.999 / 0.999 / 0.998 / 0.988   0.999 / 0.999 / 0.997 / 0.998
  bf16-scalar-d48           0.999 / 0.999 / 0.999 / 0.996   0.999 / 0.999 / 0.999 / 0.996
  CorrBlock f32 nchw        -                               0.204 / 0.154 / 0.139 / 0.059
  CorrBlock f32 nhwc        -                               0.204 / 0.154 / 0.139 / 0.059
  CorrBlock bf16 nchw       -                               0.999 / 0.999 / 0.999 / 0.992
  CorrBlock bf16 nhwc       -                               0.999 / 0.999 / 0.999 / 0.992
  CorrBlock f16 nchw        -                               0.228 / 0.171 / 0.140 / 0.054
  CorrBlock f16 nhwc        -                               0.228 / 0.171 / 0.140 / 0.054

num_levels 1..3 (dma-nchw, pack-dma16-bf16) reproduce the first levels of the four-level rows.

A finding: float16 fmaps whose values reach float16's subnormal range.  Under the
documented contract alone (one exact product per element, a chain of 2 D / 32 + 17
roundings) the float16 record builds left 3 of the 32,400 level-0 cells of ``ragged`` on
``wide`` data outside the bound, at 1.89, 1.63 and 1.02 of it (43, 38 and 23 u M; the
host emulation uses 3.5), in cells that pair pixels most of whose channels are float16
subnormals; the bfloat16 records of the same data stay at 0.21.  Measured one instruction
at a time, v_mfma_f32_32x32x16_f16 aligns a subnormal operand by its format's exponent
2^-14 and cuts every addend 24 bits below the largest such nominal product, so
corr_build_dma_kernel's comment on OPK = DMA_F16 ("the f32 matmul of the widened fmaps to
accumulation rounding ... no scales") does not hold for such fmaps.  build_oracle counts
that as 17 u (Mn - M) for float16 operands (its module docstring has the measurements and
the reasoning); operands in the normal range keep the bound as it was, and the rows above
are measured with the term in place.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import build_oracle as bo

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


@pytest.fixture(scope="module")
def dx():
    import dexiraft_amd
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    dexiraft_amd.load_native()
    return dexiraft_amd


def _fmaps(c, operand, layout):
    """The case's fmaps on the device as the request's type and layout (the
    values are the operand type's already: the conversion is exact)."""
    out = []
    for f in (c.f1, c.f2):
        t = torch.from_numpy(np.array(f)).to(DEV).to(TORCH[operand])
        assert torch.equal(t.float().cpu(), torch.from_numpy(np.array(f)))
        if layout == "nhwc":
            t = t.contiguous(memory_format=torch.channels_last)
        out.append(t)
    return out


def _build(r, c, L=4):
    """The request through the C ABI into a NaN-filled pyramid; the levels as
    float64 arrays [B*N, H_l, W_l]."""
    from dexiraft_amd import _native as nat
    lib = nat.load()
    B, D, H, W = c.B, c.D, c.H, c.W
    f1, f2 = _fmaps(c, r.operand, r.layout)
    in_dt = {"f32": nat.DXR_F32, "bf16": nat.DXR_BF16, "f16": nat.DXR_F16}[r.operand]
    pyr_dt = {"f32": nat.DXR_F32, "bf16": nat.DXR_BF16, "f16": nat.DXR_PYR_F16}[r.cells]
    lay = nat.DXR_NHWC if r.layout == "nhwc" else nat.DXR_NCHW
    algo = nat.DXR_BUILD_EXACT_F32 if r.algo == "exact" else nat.DXR_BUILD_AUTO
    buf = torch.full((lib.dxr_pyramid_numel(B, H, W, L),), float("nan"), device=DEV,
                     dtype=TORCH[r.cells])
    s = nat.stream_of(f1)
    div = float(c.div)
    if r.ws:
        nb = max(lib.dxr_build_workspace_bytes(in_dt, B, D, H, W), 0)
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=DEV)
        st = lib.dxr_corr_pyramid_build_ws(f1.data_ptr(), f2.data_ptr(), in_dt, lay, B, D, H, W, L,
                                           div, buf.data_ptr(), pyr_dt, algo, ws.data_ptr(), nb, s)
    else:
        st = lib.dxr_corr_pyramid_build(f1.data_ptr(), f2.data_ptr(), in_dt, lay, B, D, H, W, L, div,
                                        buf.data_ptr(), pyr_dt, algo, s)
    assert st == 0, st
    got = []
    for lvl, (h, w) in enumerate(bo.level_shapes(H, W, L)):
        t = torch.full((B * H * W, h, w), float("nan"), device=DEV)
        assert lib.dxr_pyramid_unpack(buf.data_ptr(), pyr_dt, B, H, W, L, lvl, t.data_ptr(), s) == 0
        got.append(t.cpu().numpy().astype(np.float64))
    return got


def _hold(tag, c, family, cells, got, L=4):
    fr = bo.check(c, family, cells, got, L)
    print(f"BUILD-PER-CELL {tag}: " + " / ".join(f"{x:.3f}" for x in fr) + " of the bound")
    assert max(fr) <= 1.0, (tag, fr)


@pytest.mark.parametrize("kind", bo.KINDS)
@pytest.mark.parametrize("r", bo.REQUESTS, ids=[r.id for r in bo.REQUESTS])
def test_every_cell_of_every_level(dx, r, kind):
    c = bo.request_case(r, kind)
    _hold(f"{r.id} {kind}", c, r.family, r.cells, _build(r, c))


@pytest.mark.parametrize("L", (1, 2, 3))
@pytest.mark.parametrize("r", bo.LEVEL_REQUESTS, ids=[r.id for r in bo.LEVEL_REQUESTS])
def test_fewer_levels(dx, r, L):
    """num_levels 1..3: the epilogue's early returns sit between its staging barriers."""
    for kind in bo.KINDS:
        c = bo.request_case(r, kind)
        _hold(f"{r.id} L={L} {kind}", c, r.family, r.cells, _build(r, c, L), L)


@pytest.mark.parametrize("layout", ("nchw", "nhwc"))
@pytest.mark.parametrize("operand", ("f32", "bf16", "f16"))
def test_through_corrblock(dx, operand, layout):
    """CorrBlock's own planner arguments (workspace, alignment, layout) on ``wide``
    data: f32 fmaps take the pre-split DMA build, bf16 and float16 fmaps the
    16-bit record builds (D = 96), under the same bounds."""
    c = bo.case("ragged", 96, "wide", operand)
    f1, f2 = _fmaps(c, operand, layout)
    cb = dx.CorrBlock(f1, f2)
    got = [lv[:, 0].cpu().numpy().astype(np.float64) for lv in cb.corr_pyramid]
    family = "pair_scaled" if operand == "f32" else "rec16"
    cells = "bf16" if operand == "bf16" else "f32"
    _hold(f"CorrBlock {operand} {layout}", c, family, cells, got)
