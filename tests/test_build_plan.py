"""CPU: which kernel serves which pyramid build request.

csrc/build_plan.h is the planner behind dxr_corr_pyramid_build / _build_ws.
tests/cpp/build_plan_table.cpp, a stand-alone host program that includes only
that header, is compiled with ASan + UBSan and run on the requests below; the
expected status and kernel of every row are written out by hand from the
"Kernels by request" table of include/dexiraft_corr.h, not produced by the
planner.  Rows that are refused (and B == 0) are also sent through the C-ABI
with dummy addresses and must answer the same status; rows that would launch
are not, so no GPU is needed.
"""
from __future__ import annotations

import importlib.util
import re
import subprocess

import pytest

from conftest import REPO

CSRC = REPO / "optical-flow_dexi-raft_amd" / "csrc"
HEADER = REPO / "include" / "dexiraft_corr.h"

OK, EINVAL, EUNSUP = 0, 1, 2
F32, BF16, F16, PYR_F16 = 0, 1, 2, 4
NCHW, NHWC = 0, 1
AUTO, EXACT = 0, 1

# kernel names, as the header's table spells them
DMA_NCHW = "split_pairs_kernel<NCHW> + corr_build_dma_kernel"
DMA_NHWC = "split_pairs_kernel<NHWC> + corr_build_dma_kernel"
SPLIT_F4 = "corr_build_split_kernel<float4>"
SPLIT_F2 = "corr_build_split_kernel<float2>"
SPLIT_NHWC = "corr_build_split_kernel<NHWC>"
EXACT_VEC = "corr_build_f32_kernel<vec>"
EXACT_SCALAR = "corr_build_f32_kernel<scalar>"
PACK_DMA16 = "pack_bf16_kernel + corr_build_dma_kernel"
DMA16_NHWC = "corr_build_dma_kernel"
BF16_Q2 = "corr_build_bf16_q2_kernel"
BF16_ONE = "corr_build_bf16_kernel"
NONE = "none"
ALL_PATHS = {DMA_NCHW, DMA_NHWC, SPLIT_F4, SPLIT_F2, SPLIT_NHWC, EXACT_VEC, EXACT_SCALAR,
             PACK_DMA16, DMA16_NHWC, BF16_Q2, BF16_ONE}

A16, A8, A4, A2 = 0x10000, 0x10008, 0x10004, 0x10002   # dummy addresses by alignment
WS16, WS8 = 0x40000, 0x40008


def ws_bytes(dt, B, D, H, W):
    """dxr_build_workspace_bytes as the header documents it (-1 beyond int64)."""
    al = lambda x: (x + 255) // 256 * 256   # noqa: E731
    if B < 0 or D < 1 or H < 1 or W < 1 or H * W > 1 << 30:
        return -1
    if dt in (BF16, F16):
        n = 2 * al(B * D * H * W * 2) if D % 32 == 0 else 0
    elif dt == F32 and D % 16 == 0:
        n = 2 * al(B * D * H * W * 4) + 2 * al(B * H * W * 4)
    else:
        n = 0
    return n if n < 1 << 63 else -1


def rq(dt=F32, lay=NCHW, B=1, D=64, H=23, W=32, L=4, div=8.0, pyr=None, algo=AUTO,
       f1=A16, f2=A16, p=A16, ws=None, dhw=None):
    """One request.  pyr None: the fmaps' own type (f16 fmaps: f32).  ws: None (no
    workspace), "exact", "short" (one byte less), "a8" (exact size, 8-byte
    aligned only).  dhw: what D * H * W is meant to be (checked)."""
    if pyr is None:
        pyr = {F32: F32, BF16: BF16, F16: F32}.get(dt, F32)
    assert dhw is None or D * H * W == dhw
    need = max(ws_bytes(dt, B, D, H, W), 0)
    wa, wb = {None: (0, 0), "exact": (WS16, need), "short": (WS16, need - 1),
              "a8": (WS8, need)}[ws]
    return dict(dt=dt, lay=lay, B=B, D=D, H=H, W=W, L=L, div=div, pyr=pyr, algo=algo,
                f1=f1, f2=f2, p=p, ws=wa, wsb=wb)


def rows():
    """(request, status, kernel[, pool_extra]) — by hand from the header's table."""
    t = []

    def add(r, st, path=NONE, pool=0):
        t.append((r, st, path, pool))

    # --- D in {16, 24, 32, 48}: % 16 and % 32 (48: % 16 only) -------------------
    for D, nows, withws in ((16, SPLIT_F4, DMA_NCHW), (24, EXACT_VEC, EXACT_VEC),
                            (32, SPLIT_F4, DMA_NCHW), (48, SPLIT_F4, DMA_NCHW)):
        add(rq(D=D), OK, nows)
        add(rq(D=D, ws="exact"), OK, withws)
    for D, nows, withws in ((16, SPLIT_NHWC, DMA_NHWC), (24, None, None),
                            (32, SPLIT_NHWC, DMA_NHWC), (48, SPLIT_NHWC, DMA_NHWC)):
        for ws, want in ((None, nows), ("exact", withws)):
            add(rq(lay=NHWC, D=D, ws=ws), *((OK, want) if want else (EUNSUP,)))
    for D in (16, 24, 32, 48):
        stage = D % 32 == 0
        add(rq(BF16, D=D), OK, BF16_Q2)
        add(rq(BF16, D=D, ws="exact"), OK, PACK_DMA16 if stage else BF16_Q2)
        add(rq(BF16, NHWC, D=D), *((OK, DMA16_NHWC) if stage else (EUNSUP,)))
        add(rq(F16, NHWC, D=D), *((OK, DMA16_NHWC) if stage else (EUNSUP,)))
        add(rq(F16, D=D, ws="exact"), *((OK, PACK_DMA16) if stage else (EUNSUP,)))
        add(rq(F16, D=D), EUNSUP)

    # --- W in {30, 31, 32}: even but not % 4, odd, % 4 --------------------------
    for W, nchw, nhwc, exact, bf in ((30, SPLIT_F2, SPLIT_NHWC, EXACT_SCALAR, BF16_ONE),
                                     (31, EXACT_SCALAR, None, EXACT_SCALAR, BF16_ONE),
                                     (32, SPLIT_F4, SPLIT_NHWC, EXACT_VEC, BF16_Q2)):
        add(rq(W=W), OK, nchw)
        add(rq(W=W, ws="exact"), OK, DMA_NCHW)                  # the DMA build takes any W
        add(rq(lay=NHWC, W=W), *((OK, nhwc) if nhwc else (EUNSUP,)))
        add(rq(lay=NHWC, W=W, ws="exact"), OK, DMA_NHWC)
        add(rq(W=W, algo=EXACT), OK, exact)
        add(rq(BF16, W=W), OK, bf)

    # --- workspace: null, one byte short, exact, exact but 8-byte aligned -------
    for ws, has in ((None, False), ("short", False), ("exact", True), ("a8", False)):
        add(rq(ws=ws), OK, DMA_NCHW if has else SPLIT_F4)
        add(rq(lay=NHWC, ws=ws), OK, DMA_NHWC if has else SPLIT_NHWC)
        add(rq(BF16, ws=ws), OK, PACK_DMA16 if has else BF16_Q2)
        add(rq(F16, ws=ws), *((OK, PACK_DMA16) if has else (EUNSUP,)))
        add(rq(pyr=PYR_F16, ws=ws), *((OK, DMA_NCHW) if has else (EUNSUP,)))
        add(rq(lay=NHWC, pyr=PYR_F16, ws=ws), *((OK, DMA_NHWC) if has else (EUNSUP,)))
        add(rq(F16, pyr=PYR_F16, ws=ws), *((OK, PACK_DMA16) if has else (EUNSUP,)))

    # --- pyramid 8-byte aligned only, on every path that demands 16 --------------
    add(rq(p=A8, ws="exact"), OK, EXACT_SCALAR)       # no DMA, no split: exact, scalar staging
    add(rq(p=A8), OK, EXACT_SCALAR)
    add(rq(p=A8, W=30), OK, EXACT_SCALAR)             # float2 units need it too
    add(rq(p=A8, algo=EXACT), OK, EXACT_SCALAR)
    add(rq(lay=NHWC, p=A8, ws="exact"), EUNSUP)
    add(rq(lay=NHWC, p=A8), EUNSUP)
    add(rq(BF16, p=A8, ws="exact"), OK, BF16_ONE)
    add(rq(BF16, p=A8), OK, BF16_ONE)
    add(rq(BF16, NHWC, p=A8), EUNSUP)
    add(rq(F16, NHWC, p=A8), EUNSUP)
    add(rq(F16, p=A8, ws="exact"), EUNSUP)
    add(rq(pyr=PYR_F16, p=A8, ws="exact"), EUNSUP)

    # --- fmaps 8-byte (4-byte) aligned only ---------------------------------------
    add(rq(lay=NHWC, f1=A8, ws="exact"), EUNSUP)      # not the DMA build; the split wants 16 too
    add(rq(lay=NHWC, f2=A8, ws="exact"), EUNSUP)
    add(rq(lay=NHWC, f1=A8), EUNSUP)
    add(rq(lay=NHWC, pyr=PYR_F16, f1=A8, ws="exact"), EUNSUP)
    add(rq(BF16, NHWC, f1=A8), EUNSUP)
    add(rq(F16, NHWC, f2=A8), EUNSUP)
    add(rq(BF16, f1=A8), OK, BF16_Q2)
    add(rq(BF16, f1=A8, f2=A4), OK, BF16_ONE)
    add(rq(BF16, f1=A4), OK, BF16_ONE)
    add(rq(f1=A8), OK, SPLIT_F2)                      # W = 32, but float4 units want 16
    add(rq(f2=A4), OK, EXACT_SCALAR)
    add(rq(f1=A4, ws="exact"), OK, DMA_NCHW)          # NCHW rows are read as scalars
    add(rq(BF16, f1=A2, ws="exact"), OK, PACK_DMA16)  # the pack pass reads any alignment
    add(rq(F16, f1=A2, ws="exact"), OK, PACK_DMA16)

    # --- 4 levels against 5 (levels beyond 4: f32 pooling passes) ----------------
    big = dict(H=32, W=32)
    for L in (4, 5):
        more = L == 5
        add(rq(L=L, **big), OK, SPLIT_F4, more)
        add(rq(L=L, ws="exact", **big), OK, DMA_NCHW, more)
        add(rq(lay=NHWC, L=L, ws="exact", **big), OK, DMA_NHWC, more)
        add(rq(L=L, pyr=BF16, **big), *((EUNSUP,) if more else (OK, SPLIT_F4)))
        add(rq(L=L, pyr=PYR_F16, ws="exact", **big), *((EUNSUP,) if more else (OK, DMA_NCHW)))
        add(rq(BF16, L=L, **big), *((EUNSUP,) if more else (OK, BF16_Q2)))
        # bf16 NCHW with a workspace, f32 pyramid: five levels skip the pack path
        add(rq(BF16, L=L, pyr=F32, ws="exact", **big), OK, BF16_Q2 if more else PACK_DMA16, more)
        add(rq(BF16, L=L, pyr=F32, ws="exact", f1=A4, **big), OK,
            BF16_ONE if more else PACK_DMA16, more)
        add(rq(BF16, NHWC, L=L, pyr=F32, **big), OK, DMA16_NHWC, more)
        add(rq(F16, NHWC, L=L, **big), OK, DMA16_NHWC, more)
        add(rq(F16, L=L, ws="exact", **big), OK, PACK_DMA16, more)
        add(rq(F16, NHWC, L=L, pyr=PYR_F16, **big), *((EUNSUP,) if more else (OK, DMA16_NHWC)))
    add(rq(L=0), EINVAL)
    add(rq(L=9), EINVAL)
    add(rq(H=7, W=30), EINVAL)                        # 7 -> 3 -> 1 -> 0 rows
    add(rq(H=8, W=8), OK, SPLIT_F4)

    # --- DXR_BUILD_EXACT_F32 -------------------------------------------------------
    add(rq(algo=EXACT), OK, EXACT_VEC)
    add(rq(algo=EXACT, ws="exact"), OK, EXACT_VEC)
    add(rq(lay=NHWC, algo=EXACT), EUNSUP)
    add(rq(lay=NHWC, algo=EXACT, ws="exact"), EUNSUP)
    add(rq(BF16, algo=EXACT), EUNSUP)
    add(rq(F16, NHWC, algo=EXACT), EUNSUP)            # decided before the f16 rows
    add(rq(pyr=PYR_F16, algo=EXACT, ws="exact"), EUNSUP)
    # pyramid types that a fmap type cannot have
    add(rq(F16, NHWC, pyr=BF16), EUNSUP)
    add(rq(BF16, NHWC, pyr=PYR_F16), EUNSUP)
    add(rq(BF16, pyr=PYR_F16, ws="exact"), EUNSUP)
    add(rq(BF16, pyr=F32), OK, BF16_Q2)
    add(rq(pyr=BF16), OK, SPLIT_F4)
    add(rq(pyr=BF16, ws="exact"), OK, DMA_NCHW)

    # --- size limits: D*H*W < 2^29 (f32 split forms), < 2^30 (16-bit forms) -------
    # D % 16 == 0 makes 2^29 - 16 the largest product below the limit (- 32 with
    # an even W, - 64 with W % 4 == 0), D % 32 == 0 makes it 2^30 - 32; the literal
    # 2^29 - 1 and 2^30 - 1 are odd, so they only reach kernels without a limit.
    lo29 = dict(D=496, H=601, W=1801, L=1, dhw=2**29 - 16)
    ev29 = dict(D=240, H=273, W=8194, L=1, dhw=2**29 - 32)
    v29 = dict(D=752, H=178481, W=4, L=1, dhw=2**29 - 64)
    at29 = dict(D=128, H=2048, W=2048, L=1, dhw=2**29)
    add(rq(ws="exact", **lo29), OK, DMA_NCHW)
    add(rq(lay=NHWC, ws="exact", **lo29), OK, DMA_NHWC)
    add(rq(pyr=PYR_F16, ws="exact", **lo29), OK, DMA_NCHW)
    add(rq(**ev29), OK, SPLIT_F2)
    add(rq(lay=NHWC, **ev29), OK, SPLIT_NHWC)
    add(rq(**v29), OK, SPLIT_F4)
    add(rq(ws="exact", **at29), OK, EXACT_VEC)
    add(rq(**at29), OK, EXACT_VEC)
    add(rq(lay=NHWC, ws="exact", **at29), EUNSUP)
    add(rq(lay=NHWC, **at29), EUNSUP)
    add(rq(pyr=PYR_F16, ws="exact", **at29), EUNSUP)
    add(rq(D=233, H=1103, W=2089, L=1, dhw=2**29 - 1), OK, EXACT_SCALAR)
    lo30 = dict(D=992, H=601, W=1801, L=1, dhw=2**30 - 32)
    at30 = dict(D=256, H=2048, W=2048, L=1, dhw=2**30)
    for dt in (BF16, F16):
        add(rq(dt, NHWC, **lo30), OK, DMA16_NHWC)
        add(rq(dt, NHWC, **at30), EUNSUP)
        add(rq(dt, ws="exact", **lo30), OK, PACK_DMA16)
    add(rq(F16, ws="exact", **at30), EUNSUP)
    add(rq(BF16, ws="exact", **at30), OK, BF16_ONE)   # neither the pack path nor q2
    add(rq(BF16, **at30), OK, BF16_ONE)
    add(rq(BF16, D=435, H=4859, W=508, L=1, dhw=2**30 - 4), OK, BF16_Q2)
    add(rq(BF16, D=693, H=4681, W=331, L=1, dhw=2**30 - 1), OK, BF16_ONE)
    add(rq(D=1 << 20, H=8, W=8, L=1), OK, SPLIT_F4)
    add(rq(D=(1 << 20) + 16, H=8, W=8, L=1), EINVAL)
    add(rq(H=1 << 15, W=(1 << 15) + 1, D=16, L=1), EINVAL)        # H*W > 2^30

    # --- ceil(H*W / 128) > 65535 rows of the 3-D grid -----------------------------
    rows_ok = dict(D=16, H=65535, W=128)          # 65535 rows
    rows_over = dict(D=16, H=4096, W=2048)        # 65536 rows
    add(rq(**rows_ok), OK, SPLIT_F4)
    add(rq(**rows_over), EINVAL)
    add(rq(ws="exact", **rows_over), EINVAL)
    add(rq(lay=NHWC, **rows_over), EINVAL)
    add(rq(algo=EXACT, **rows_over), EINVAL)
    add(rq(BF16, **rows_over), EINVAL)
    add(rq(BF16, f1=A4, **rows_over), EINVAL)
    add(rq(lay=NHWC, f1=A8, **rows_over), EUNSUP)                 # unsupported comes first
    over32 = dict(rows_over, D=32)
    add(rq(BF16, NHWC, **over32), OK, DMA16_NHWC)                 # 1-D grids: no such bound
    add(rq(F16, NHWC, **over32), OK, DMA16_NHWC)
    add(rq(BF16, ws="exact", **over32), OK, PACK_DMA16)
    add(rq(F16, ws="exact", **over32), OK, PACK_DMA16)

    # --- argument checks -------------------------------------------------------------
    add(rq(B=0, f1=0, f2=0, p=0), OK)                             # before the pointers
    add(rq(BF16, B=0, L=5, H=32, f1=0, f2=0, p=0), OK)            # and before "unsupported"
    add(rq(B=0, D=0), EINVAL)
    add(rq(B=0, algo=9), EINVAL)
    add(rq(B=65535, D=16, H=8, W=8, L=1), OK, SPLIT_F4)
    add(rq(B=65535, D=16, H=8, W=8, L=1, ws="exact"), OK, DMA_NCHW)
    add(rq(B=65536, D=16, H=8, W=8, L=1), EINVAL)
    add(rq(B=-1), EINVAL)
    add(rq(div=0.0), EINVAL)
    add(rq(div=float("nan")), EINVAL)
    add(rq(D=0), EINVAL)
    add(rq(dt=7), EINVAL)
    add(rq(dt=PYR_F16), EINVAL)                                   # a pyr_dtype only
    add(rq(pyr=3), EINVAL)
    add(rq(pyr=7), EINVAL)
    add(rq(pyr=F16), EINVAL)                                      # an in_dtype only
    add(rq(F16, NHWC, pyr=F16), EINVAL)
    add(rq(lay=2), EINVAL)
    add(rq(algo=9), EINVAL)
    add(rq(f1=0), EINVAL)
    add(rq(f2=0), EINVAL)
    add(rq(p=0), EINVAL)
    add(rq(BF16, L=5, H=32, f1=0), EINVAL)                        # invalid before unsupported
    add(rq(BF16, algo=EXACT, p=0), EINVAL)
    add(rq(BF16, algo=9, L=5, H=32), EINVAL)

    # --- dxr_build_workspace_bytes beyond int64 (the requests themselves: B, D, H*W) ---
    add(rq(B=1 << 62, D=16, H=1, W=1, L=1), EINVAL)
    add(rq(B=1 << 30, D=1 << 20, H=32, W=32, L=1), EINVAL)        # 4 B D N = 2^62, doubled
    add(rq(BF16, B=1 << 31, D=1 << 21, H=1 << 5, W=1 << 5, L=1), EINVAL)
    add(rq(F16, B=65535, D=1 << 20, H=1 << 15, W=1 << 15, L=1, lay=NHWC), EUNSUP)
    add(rq(B=3, D=(1 << 62) + 16, H=1, W=1, L=1), EINVAL)
    add(rq(B=1, D=16, H=1 << 40, W=1 << 40, L=1), EINVAL)

    # --- the requests of tests/test_gpu_build_per_cell.py, at its shapes (16-byte
    # aligned buffers, as torch allocates them): each reaches the kernel its bound is for
    import build_oracle as bo
    code = {"f32": F32, "bf16": BF16, "f16": F16}
    for r in bo.REQUESTS:
        B, H, W = bo.CASES[r.case]
        for L in (1, 2, 3, 4) if r in bo.LEVEL_REQUESTS else (4,):
            add(rq(code[r.operand], NHWC if r.layout == "nhwc" else NCHW, B=B, D=r.D, H=H, W=W, L=L,
                   pyr=PYR_F16 if r.cells == "f16" else code[r.cells],
                   algo=EXACT if r.algo == "exact" else AUTO, ws="exact" if r.ws else None),
                OK, r.path)
    return t


TABLE = rows()


def _line(r):
    div = "nan" if r["div"] != r["div"] else repr(float(r["div"]))
    return " ".join(str(x) for x in (r["dt"], r["lay"], r["B"], r["D"], r["H"], r["W"], r["L"], div,
                                     r["pyr"], r["algo"], r["f1"], r["f2"], r["p"], r["ws"],
                                     r["wsb"]))


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """The planner's answers for TABLE: the sanitized program's output, parsed."""
    spec = importlib.util.spec_from_file_location(
        "_dxr_build_p", REPO / "optical-flow_dexi-raft_amd" / "build.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    d = tmp_path_factory.mktemp("build_plan")
    exe, req = d / "build_plan_table", d / "requests.txt"
    subprocess.run([b.hipcc(), "-x", "c++", "-std=c++17", "-O1", "-g",
                    "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover",
                    f"-I{REPO / 'include'}", f"-I{CSRC}",
                    str(REPO / "tests" / "cpp" / "build_plan_table.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    req.write_text("".join(_line(r) + "\n" for r, *_ in TABLE))
    res = subprocess.run([str(exe), str(req)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    out = []
    for ln in res.stdout.splitlines():
        st, name, nbytes, rest = ln.split("\t")
        operand, cells, pool = (int(x) for x in rest.split())
        out.append((int(st), name, int(nbytes), operand, cells, pool))
    assert len(out) == len(TABLE)
    return out


def test_planner_includes_no_hip():
    """The planner is host-only: its header pulls in nothing of HIP."""
    incs = re.findall(r'#include\s+[<"]([^>"]+)[>"]', (CSRC / "build_plan.h").read_text())
    assert incs and all("hip" not in i and i != "dxr_common.h" for i in incs), incs
    prog = (REPO / "tests" / "cpp" / "build_plan_table.cpp").read_text()
    assert [i for i in re.findall(r'#include\s+"([^"]+)"', prog)] == ["build_plan.h"]


def test_table_covers_every_kernel_row_of_the_header():
    """Every kernel name the rows expect stands in the header's table, and the
    rows reach every build path."""
    table = HEADER.read_text().split("Kernels by request", 1)[1].split("*/", 1)[0]
    for name in ALL_PATHS:
        assert name in table, name
    assert {path for _, st, path, _ in TABLE if st == OK and path != NONE} == ALL_PATHS


def test_every_row_of_the_table(planned):
    bad = []
    for i, ((r, st, path, pool), got) in enumerate(zip(TABLE, planned)):
        g_st, g_name, g_bytes, g_operand, g_cells, g_pool = got
        want_bytes = ws_bytes(r["dt"], r["B"], r["D"], r["H"], r["W"])
        if (g_st, g_name, g_bytes) != (st, path, want_bytes):
            bad.append((i, _line(r), (st, path, want_bytes), got))
        elif st == OK and path != NONE and (g_operand, g_cells, g_pool) != (r["dt"], r["pyr"],
                                                                              int(pool)):
            bad.append((i, _line(r), (r["dt"], r["pyr"], int(pool)), got))
    assert not bad, "\n".join(map(str, bad))


def test_workspace_bytes_documented_values_and_overflow(planned):
    """dxr_build_workspace_bytes through the C-ABI: the planner's value for every
    row (they share the size functions), the documented sizes, and -1 where the
    size would not fit int64."""
    from dexiraft_amd import _native as nat
    lib = nat.load()
    wsb = lib.dxr_build_workspace_bytes
    for (r, *_), got in zip(TABLE, planned):
        assert wsb(r["dt"], r["B"], r["D"], r["H"], r["W"]) == got[2], _line(r)
    al = lambda x: (x + 255) // 256 * 256   # noqa: E731
    assert wsb(F32, 2, 64, 13, 19) == 2 * al(2 * 64 * 247 * 4) + 2 * al(2 * 247 * 4)
    assert wsb(BF16, 1, 256, 55, 128) == wsb(F16, 1, 256, 55, 128) == 2 * al(256 * 7040 * 2)
    assert wsb(F32, 1, 24, 55, 128) == 0 and wsb(BF16, 1, 48, 55, 128) == 0
    assert wsb(7, 1, 64, 8, 8) == 0 and wsb(F32, 0, 64, 8, 8) == 0
    assert wsb(F32, -1, 64, 8, 8) == -1 and wsb(F32, 1, 0, 8, 8) == -1
    assert wsb(F32, 1, 64, 1 << 15, (1 << 15) + 1) == -1
    i64 = (1 << 63) - 1
    assert wsb(F32, i64, 16, 1, 1) == -1 and wsb(BF16, 1, i64 - 31, 1, 1) == -1
    assert wsb(F32, 1, 16, i64, i64) == -1
    assert wsb(F32, 1 << 30, 1 << 20, 32, 32) == -1          # 2^62 bytes per copy, two copies
    assert wsb(F32, 1 << 29, 1 << 20, 32, 32) == 2 * (1 << 61) + 2 * (1 << 41)


def test_refused_rows_answer_the_same_through_the_c_abi():
    from dexiraft_amd import _native as nat
    lib = nat.load()
    n = 0
    for r, st, path, _ in TABLE:
        if st == OK and path != NONE:
            continue            # would launch
        if not -(1 << 63) <= r["B"] < 1 << 63 or r["D"] >= 1 << 63:
            continue
        head = (r["f1"] or None, r["f2"] or None, r["dt"], r["lay"], r["B"], r["D"], r["H"],
                r["W"], r["L"], r["div"], r["p"] or None, r["pyr"], r["algo"])
        if r["ws"]:
            got = lib.dxr_corr_pyramid_build_ws(*head, r["ws"], r["wsb"], None)
        else:
            got = lib.dxr_corr_pyramid_build(*head, None)
        assert got == st, _line(r)
        n += 1
    assert n > 80
    assert lib.dxr_last_hip_error() == 0
