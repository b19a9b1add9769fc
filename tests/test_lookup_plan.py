"""CPU: which unit, kernel, grid and store policy serve which forward lookup.

csrc/lookup_plan.h is the planner behind dxr_corr_lookup /
dxr_corr_lookup_conv1x1 (the pyramid lookup), dxr_alt_volume_lookup (the volume
lookup) and dxr_alt_corr_lookup / _ws / _levels_ws (the on-the-fly lookup).
tests/cpp/lookup_plan_table.cpp, a stand-alone host program that includes only
that header, is compiled with ASan + UBSan and run on the requests below; the
expected status, unit, kernel, grid and store policy of every row are written
out by hand from the "Lookup kernels by request" table of
include/dexiraft_corr.h, not produced by the planner.  Rows that are refused
(and B == 0) are also sent through the C-ABI with dummy addresses and must
answer the same status; rows that would launch are not, so no GPU is needed.
Sizes are H x W at 1/8 resolution.
"""
from __future__ import annotations

import ctypes
import importlib.util
import re
import subprocess

import pytest

from conftest import REPO

CSRC = REPO / "optical-flow_dexi-raft_amd" / "csrc"
HEADER = REPO / "include" / "dexiraft_corr.h"

OK, EINVAL, EUNSUP = 0, 1, 2
F32, BF16, DT_F16, PYR_F16 = 0, 1, 2, 4
O16, OBF, ONHWC = 0x100, 0x200, 0x1000
IN16, INBF, VOL16 = 0x8000, 0x20000, 0x40000
OUT_FORMS = (0, O16, OBF, ONHWC, ONHWC | O16, ONHWC | OBF)
PINNED_INVALID = (0x400, 0x800, 0x2000, 0x4000, 0x10000, 1 << 30)
NEG = -(1 << 31)                      # or-ed in: a negative value with its low bits kept

A16, A8, ODD = 0x10000, 0x10008, 0x10001   # dummy addresses by alignment
WS16, WS8 = 0x40000, 0x40008

# units and kernel names, as the header's table spells them
U_MAIN, U_OUT16, U_PYR16, U_NHWC = ("corr_lookup.hip", "corr_lookup_out16.hip",
                                    "corr_lookup_pyr16.hip", "corr_lookup_nhwc.hip")
V_MAIN, V_OUT, V_VOL16 = "corr_lookup.hip", "corr_lookup_alt_out.hip", "corr_lookup_alt_vol16.hip"
A_MAIN, A_OUT, A_IN16, A_INBF = ("alt_corr.hip", "alt_corr_out.hip", "alt_corr_in16.hip",
                                 "alt_corr_inbf16.hip")
ONE, MULTI32, MULTI16 = ("corr_lookup_qm_kernel<256 x 16>", "corr_lookup_qm_kernel<512 x 32>",
                         "corr_lookup_qm_kernel<512 x 16>")
CONV1024, CONV512 = "corr_lookup_conv1x1_h2_kernel<1024>", "corr_lookup_conv1x1_h2_kernel<512>"
VONE, VMULTI32, VMULTI16 = ("corr_lookup_qm_kernel<ALT, 256 x 16>",
                            "corr_lookup_qm_kernel<ALT, 512 x 32>",
                            "corr_lookup_qm_kernel<ALT, 512 x 16>")
ORDERED, TILE = "alt_bin_*_kernel + alt_corr_mfma_kernel<ordered>", "alt_corr_mfma_kernel<tile order>"
VEC, SCALAR = "alt_corr_kernel<vec>", "alt_corr_kernel<scalar>"
NONE = "none"
# every (unit, kernel) of the header's table
ALL_P = {(u, k) for u in (U_MAIN, U_OUT16, U_PYR16, U_NHWC)
         for k in (ONE, MULTI32, MULTI16, CONV1024, CONV512)}
ALL_V = {(u, k) for u in (V_MAIN, V_OUT, V_VOL16) for k in (VONE, VMULTI32, VMULTI16)}
ALL_A = ({(u, k) for u in (A_MAIN, A_OUT, A_IN16, A_INBF) for k in (ORDERED, TILE)}
         | {(A_MAIN, VEC), (A_MAIN, SCALAR)})

SINTEL, CHAIRS, KITTI = (55, 128), (46, 62), (47, 156)


def ceil(a, b):
    return -(-a // b)


def p_unit(cells, form):
    """The pyramid lookup's unit, by the header's list."""
    if form & ONHWC:
        return U_NHWC
    if cells == PYR_F16:
        return U_PYR16
    return U_OUT16 if form else U_MAIN


def alt_ws_bytes(B, H, W, levels):
    """dxr_alt_workspace_bytes as the header documents it: per pair and level the
    entries int4[NP] | ids int[NP] | cnt int[64][4097] | tot int[4097] | cost
    float[64], 16-byte aligned, NP = whole 4 x 8 query tiles."""
    if B < 0 or H < 1 or W < 1 or not 1 <= levels <= 8 or H * W > 1 << 30:
        return -1
    np_ = ceil(W, 8) * ceil(H, 4) * 32
    per = (20 * np_ + 4 * 64 * 4097 + 4 * 4097 + 4 * 64 + 15) & ~15
    return B * levels * per


def rows():
    """Requests and, by hand from the header's table, what each must answer."""
    t = []

    # ---- pyramid lookup --------------------------------------------------------
    def P(dt=F32, B=1, hw=SINTEL, L=4, r=4, conv=0, cout=0, pyr=A16, coords=A16, wp=None, out=A16,
          st=OK, kernel=NONE, grid=(0, 0, 0), nt=0, unit=None):
        H, W = hw
        if wp is None:
            wp = A16 if conv else 0
        launches = st == OK and kernel != NONE
        form = dt & ~0xff if launches else 0
        exp = (st, (unit or p_unit(dt & 0xff, form)) if launches else NONE, kernel) + (
            (dt & 0xff, form & ~ONHWC, int(bool(form & ONHWC)), r, *grid,
             0 if form & ONHWC else nt) if launches else ())
        t.append(("P", dict(dt=dt, B=B, H=H, W=W, L=L, r=r, conv=conv, cout=cout, pyr=pyr,
                            coords=coords, wp=wp, out=out), exp))

    for cells in (F32, BF16, PYR_F16):
        for form in OUT_FORMS:
            dt = cells | form
            # Sintel B=1: 220 * 4 = 880 workgroups of 32: one round; N % 32 == 0
            P(dt, hw=SINTEL, kernel=ONE, grid=(440, 4, 1), nt=1)
            # Sintel B=2: 1,760: multi-round
            P(dt, B=2, hw=SINTEL, kernel=MULTI32, grid=(220, 4, 2), nt=1)
            # Chairs B=1: 90 * 4 = 360, N = 2852, N % 32 = 4, 48 MB: one round, write-through
            P(dt, hw=CHAIRS, kernel=ONE, grid=(179, 4, 1), nt=0)
            # KITTI B=1: 230 * 4 = 920 but N % 32 = 4 and 58 * 60 pages of 16384
            # cells * 4/3: 304 MB of f32, 152 MB of 2-byte cells: multi-round
            P(dt, hw=KITTI, kernel=MULTI32, grid=(230, 4, 1), nt=1)
            # 41 x 159: N = 6519 (% 32 = 23), 204 * 4 = 816 workgroups, 51 * 60 pages:
            # 133.7e6 B of 2-byte cells < 128 MiB = 134.2e6: one round; f32: twice that
            if cells == F32:
                P(dt, hw=(41, 159), kernel=MULTI32, grid=(204, 4, 1), nt=1)
            else:
                P(dt, hw=(41, 159), kernel=ONE, grid=(408, 4, 1), nt=0)
                # 42 x 157: N = 6594 (% 32 = 2), 52 * 60 pages: 136.3e6 B: multi-round
                P(dt, hw=(42, 157), kernel=MULTI32, grid=(207, 4, 1), nt=1)
            # wg32 == 1024 (64 x 128, N = 8192) and 1028 (57 x 144, N = 8208)
            P(dt, hw=(64, 128), kernel=ONE, grid=(512, 4, 1), nt=1)
            P(dt, hw=(57, 144), kernel=MULTI32, grid=(257, 4, 1), nt=1)
            # r = 5 ... 8: never one round, 16 queries per workgroup
            for r in (5, 6, 7, 8):
                P(dt, r=r, kernel=MULTI16, grid=(440, 4, 1), nt=1)
            P(dt, hw=(8, 8), r=5, kernel=MULTI16, grid=(4, 4, 1), nt=1)
            P(dt, r=9, st=EUNSUP)
            # 128 x 128 (N = 16384, 512 workgroups of 32 per level): 1 ... 8 levels
            for L, one in ((1, True), (2, True), (3, False), (5, False), (8, False)):
                P(dt, hw=(128, 128), L=L, kernel=ONE if one else MULTI32,
                  grid=(1024 if one else 512, L, 1), nt=1)
            P(dt, hw=(128, 128), L=9, st=EINVAL)
            # fused lookup + 1x1 convolution: ceil(N / 32) * B against 256
            P(dt, conv=1, cout=256, kernel=CONV1024, grid=(220, 1, 1))
            P(dt, B=2, conv=1, cout=256, kernel=CONV512, grid=(220, 2, 1))
            P(dt, hw=(64, 128), conv=1, cout=96, r=3, kernel=CONV1024, grid=(256, 1, 1))
            P(dt, hw=(57, 144), conv=1, cout=96, r=3, kernel=CONV512, grid=(257, 1, 1))
    for r in (0, 1, 2, 3):
        P(r=r, kernel=ONE, grid=(440, 4, 1), nt=1)
    P(hw=(7, 30), st=EINVAL)                                  # 7 -> 3 -> 1 -> 0 rows
    P(L=0, st=EINVAL)
    P(r=-1, st=EINVAL)
    P(B=65535, hw=(8, 8), L=1, kernel=MULTI32, grid=(2, 1, 65535), nt=1)
    P(B=65536, hw=(8, 8), L=1, st=EINVAL)
    P(B=-1, st=EINVAL)
    P(hw=(1 << 15, (1 << 15) + 1), L=1, st=EINVAL)            # H*W > 2^30
    P(hw=(1 << 40, 1 << 40), L=1, st=EINVAL)
    P(B=0, pyr=0, coords=0, out=0)                            # before the pointers
    P(DT_F16, B=0)                                            # and before the cell type
    P(7, B=0)
    P(DT_F16, st=EINVAL)                                      # an in_dtype of the builds only
    P(3, st=EINVAL)
    P(7, st=EINVAL)
    P(pyr=0, st=EINVAL)
    P(coords=0, st=EINVAL)
    P(out=0, st=EINVAL)
    P(conv=1, cout=256, wp=0, st=EINVAL)                      # null weight_packed
    P(conv=1, cout=256, wp=0, B=0)
    # the fused call's own limits
    for r in (0, 2, 5, 8, 9):
        P(conv=1, cout=256, r=r, st=EUNSUP)
    P(conv=1, cout=256, hw=(128, 128), L=5, st=EUNSUP)
    P(conv=1, cout=48, st=EUNSUP)
    P(conv=1, cout=4128, st=EUNSUP)
    P(conv=1, cout=4096, kernel=CONV1024, grid=(220, 1, 1))
    P(conv=1, cout=0, st=EINVAL)
    P(conv=1, cout=-32, st=EINVAL)
    # cout is the convolution's output width: independent of the lookup's channels, which
    # with <= 4 levels always fit the kernel's staged MotionCfg<R>::KP (r = 4: 336, r = 3: 208)
    P(conv=1, cout=352, kernel=CONV1024, grid=(220, 1, 1))
    P(conv=1, cout=224, r=3, kernel=CONV1024, grid=(220, 1, 1))
    P(conv=1, cout=256, L=1, hw=(8, 8), kernel=CONV1024, grid=(2, 1, 1))
    # flag errors
    for conv in (0, 1):
        kw = dict(conv=conv, cout=256 * conv)
        for bad in PINNED_INVALID + (IN16, INBF, VOL16):
            for B in (0, 1):
                P(bad | BF16, B=B, st=EINVAL, **kw)
                P(bad | O16 | BF16, B=B, st=EINVAL, **kw)
        for both in (O16 | OBF, ONHWC | O16 | OBF):
            P(both | F32, B=0, st=EINVAL, **kw)
        for form in OUT_FORMS[1:]:
            P(form | DT_F16, B=0, st=EINVAL, **kw)            # a flag on a value that is no cell type
            P(form | 7, st=EINVAL, **kw)
            P(NEG | form | BF16, st=EINVAL, **kw)             # flags on a negative value
        P(-1, B=0, st=EINVAL, **kw)
        for form in (O16, OBF, ONHWC | O16, ONHWC | OBF):
            P(form | F32, B=0, out=ODD, st=EINVAL, **kw)      # a 16-bit out at an odd address
            P(form | F32, B=0, out=ODD + 1, **kw)
        P(ONHWC | F32, B=0, out=ODD, **kw)                    # float32 elements: not checked here
        # invalid in two ways: what comes first answers
        P(0x400 | F32, r=9, st=EINVAL, **kw)
        P(0x400 | F32, L=9, B=0, st=EINVAL, **kw)
        P(O16 | F32, out=ODD, r=9, st=EINVAL, **kw)
        P(r=9, L=9, st=EINVAL, **kw)
        P(r=9, B=65536, st=EUNSUP, **kw)
        P(r=9, B=0, st=EUNSUP, **kw)
        P(r=9, pyr=0, st=EUNSUP, **kw)
        P(7, r=9, st=EUNSUP, **kw)                            # the unflagged cell type is looked at last
        P(7, pyr=0, st=EINVAL, **kw)
        P(B=65536, pyr=0, st=EINVAL, **kw)
    P(conv=1, cout=0, r=5, st=EINVAL)
    P(conv=1, cout=48, B=65536, st=EUNSUP)
    P(conv=1, cout=48, r=-1, st=EINVAL)

    # ---- volume lookup ---------------------------------------------------------
    def V(r=4, B=1, hw=SINTEL, L=4, first=2, div=8.0, vol=A16, coords=A16, out=A16, st=OK,
          kernel=NONE, grid=(0, 0, 0), nt=0):
        H, W = hw
        launches = st == OK and kernel != NONE
        form = r & (O16 | OBF | ONHWC)
        unit = V_VOL16 if r & VOL16 else V_OUT if form else V_MAIN
        exp = (st, unit if launches else NONE, kernel) + (
            (PYR_F16 if r & VOL16 else F32, form & ~ONHWC, int(bool(form & ONHWC)), r & 0xff,
             *grid, 0 if form & ONHWC else nt) if launches else ())
        t.append(("V", dict(B=B, H=H, W=W, L=L, first=first, r=r, div=div, vol=vol, coords=coords,
                            out=out), exp))

    for cells in (0, VOL16):
        for form in OUT_FORMS:
            f = cells | form
            # KITTI, all four levels: 920 workgroups, N % 32 = 4, a 304 MB pyramid's worth of
            # cells — the pyramid rule goes multi-round, this one has no such exception
            V(f | 4, hw=KITTI, first=0, kernel=VONE, grid=(459, 4, 1), nt=0)
            V(f | 4, hw=KITTI, first=1, kernel=VONE, grid=(459, 3, 1), nt=0)
            V(f | 4, hw=KITTI, first=3, kernel=VONE, grid=(459, 1, 1), nt=0)
            V(f | 4, hw=KITTI, first=4, st=EINVAL)
            V(f | 4, hw=KITTI, first=5, st=EINVAL)
            V(f | 4, hw=KITTI, first=-1, st=EINVAL)
            V(f | 4, hw=SINTEL, first=2, kernel=VONE, grid=(440, 2, 1), nt=1)
            # Sintel B=8, levels 2 and 3: 220 * 2 * 8 = 3,520: multi-round; B=2, all levels: 1,760
            V(f | 4, B=8, hw=SINTEL, first=2, kernel=VMULTI32, grid=(220, 2, 8), nt=1)
            V(f | 4, B=2, hw=SINTEL, first=0, kernel=VMULTI32, grid=(220, 4, 2), nt=1)
            # wg32 == 1024 and 1028
            V(f | 4, hw=(64, 128), first=0, kernel=VONE, grid=(512, 4, 1), nt=1)
            V(f | 4, hw=(57, 144), first=0, kernel=VMULTI32, grid=(257, 4, 1), nt=1)
            for r in (0, 3):
                V(f | r, kernel=VONE, grid=(440, 2, 1), nt=1)
            for r in (5, 8):
                V(f | r, kernel=VMULTI16, grid=(440, 2, 1), nt=1)
            V(f | 9, st=EUNSUP)
            V(f | 255, B=0, st=EUNSUP)
            V(f | 4, B=0, vol=0, coords=0, out=0)
            V(f | 4, vol=0, st=EINVAL)
            V(f | 4, coords=0, st=EINVAL)
            V(f | 4, out=0, st=EINVAL)
            for bad in PINNED_INVALID + (IN16, INBF, IN16 | INBF):
                for B in (0, 1):
                    V(f | bad | 4, B=B, st=EINVAL)
            V(NEG | f | 4, st=EINVAL)                         # flags on a negative value
        for both in (O16 | OBF, ONHWC | O16 | OBF):
            V(cells | both | 4, B=0, st=EINVAL)
        for form in (O16, OBF, ONHWC | O16, ONHWC | OBF):
            V(cells | form | 4, B=0, out=ODD, st=EINVAL)
            V(cells | form | 4, B=0, out=ODD + 1)
        V(cells | ONHWC | 4, B=0, out=ODD)
        V(cells | 4, div=0.0, st=EINVAL)
        V(cells | 4, div=float("nan"), st=EINVAL)
        V(cells | 4, L=9, first=0, hw=(512, 512), st=EINVAL)
        V(cells | 4, L=8, first=7, hw=(128, 128), kernel=VONE, grid=(1024, 1, 1), nt=1)
        V(cells | 4, B=65536, st=EINVAL)
        # invalid in two ways
        V(cells | 0x400 | 9, st=EINVAL)
        V(cells | O16 | 9, out=ODD, st=EINVAL)
        V(cells | 9, first=4, st=EINVAL)
        V(cells | 9, div=0.0, st=EINVAL)
        V(cells | 9, B=65536, st=EUNSUP)
        V(cells | 9, vol=0, st=EUNSUP)
        V(cells | 4, B=65536, vol=0, st=EINVAL)
    V(-1, st=EINVAL)
    V(-1, B=0, st=EINVAL)

    # ---- on-the-fly lookup -----------------------------------------------------
    def A(r=4, B=1, hw=(16, 24), C=64, L=4, n=None, div=8.0, f1=A16, arr=A16, coords=A16, out=A16,
          ws=None, lv=None, st=OK, kernel=NONE, levels=None):
        """n None: dxr_alt_corr_lookup / _ws (every level); else _levels_ws with n_levels = n.
        ws: None, "exact", "short" (one byte less), "a8" (exact size, 8-byte aligned only), each
        for the levels the call computes.  lv: {level: address} overrides."""
        H, W = hw
        levels_call = n is not None
        nl = (n if levels_call else L)
        need = max(alt_ws_bytes(B, H, W, nl), 0) if 1 <= nl <= 8 else 0
        wa, wb = {None: (0, 0), "exact": (WS16, need), "short": (WS16, need - 1),
                  "a8": (WS8, need)}[ws]
        ptrs = [A16] * 8
        for k, v in (lv or {}).items():
            ptrs[k] = v
        launches = st == OK and kernel != NONE
        form = r & (O16 | OBF | ONHWC)
        unit = A_INBF if r & INBF else A_IN16 if r & IN16 else A_OUT if form else A_MAIN
        exp = (st, unit if launches else NONE, kernel) + (
            (form & ~ONHWC, int(bool(form & ONHWC)), r & 0xff, nl if levels is None else levels,
             int(kernel == ORDERED)) if launches else ())
        t.append(("A", dict(B=B, H=H, W=W, C=C, L=L, n=n if levels_call else -1,
                            call=int(levels_call), r=r, div=div, f1=f1, arr=arr, coords=coords,
                            out=out, ws=wa, wsb=wb, lv=ptrs), exp))

    # C: % 4 and % 16, up to 256 — and what a flagged request answers there
    for C, k in ((8, VEC), (36, VEC), (40, VEC), (64, TILE), (256, TILE), (272, VEC), (6, SCALAR),
                 (1, SCALAR), (255, SCALAR)):
        A(C=C, kernel=k)
        A(C=C, ws="exact", kernel=ORDERED if k == TILE else k)
    # fmap1 or any one level off 16-byte alignment: the scalar VALU form, whatever C
    for C in (64, 8):
        A(C=C, f1=A8, kernel=SCALAR)
        A(C=C, f1=A8, ws="exact", kernel=SCALAR)
        for l in range(4):
            A(C=C, lv={l: A8}, kernel=SCALAR)
    A(n=2, lv={2: A8}, kernel=TILE)                           # a level the call does not compute
    A(n=2, lv={3: 0}, kernel=TILE)
    A(n=2, lv={1: A8}, kernel=SCALAR)
    # the workspace: null, one byte short, exact, exact but 8-byte aligned
    for ws, has in ((None, False), ("short", False), ("exact", True), ("a8", False)):
        A(ws=ws, kernel=ORDERED if has else TILE)
        A(ws=ws, B=3, hw=(55, 128), C=256, kernel=ORDERED if has else TILE)
        A(ws=ws, n=2, kernel=ORDERED if has else TILE)        # sized for the levels computed
    # n_levels on _levels_ws
    A(n=-1, st=EINVAL)
    A(n=0, st=EINVAL)
    A(n=1, kernel=TILE)
    A(n=4, kernel=TILE)
    A(n=5, st=EINVAL)
    A(n=-1, B=0, st=EINVAL)
    A(n=0, B=0, st=EINVAL)
    A(n=5, B=0, st=EINVAL)
    A(n=4, B=0)
    # every (input flag x output form): the MFMA forms take them all, the VALU forms none
    for inp in (0, IN16, INBF):
        for form in OUT_FORMS:
            f = inp | form
            A(f | 4, kernel=TILE)
            A(f | 4, ws="exact", kernel=ORDERED)
            A(f | 4, n=2, ws="exact", kernel=ORDERED)
            if f:
                A(f | 4, C=8, st=EUNSUP)                      # C % 16 != 0
                A(f | 4, C=272, st=EUNSUP)                    # C > 256
                A(f | 4, C=6, st=EUNSUP)
                A(f | 4, f1=A8, st=EUNSUP)                    # misaligned
                A(f | 4, lv={3: A8}, ws="exact", st=EUNSUP)
                A(f | 4, C=8, B=0)                            # B == 0 comes first
                A(f | 4, C=8, lv={0: 0}, st=EINVAL)           # and so does a null level
            for r in (0, 6):
                A(f | r, kernel=TILE)
            A(f | 7, st=EUNSUP)
            A(f | 255, B=0, st=EUNSUP)
            A(f | 4, B=0, f1=0, arr=0, coords=0, out=0)
            for null in ("f1", "arr", "coords", "out"):
                A(f | 4, st=EINVAL, **{null: 0})
            A(f | 4, lv={2: 0}, st=EINVAL)
            for bad in PINNED_INVALID + (VOL16,):
                for n in (None, 2, 0):
                    A(f | bad | 4, n=n, B=0, st=EINVAL)
                A(f | bad | 4, st=EINVAL)
            A(NEG | f | 4, st=EINVAL)                         # flags on a negative value
            A(NEG | f | 4, n=0, st=EINVAL)
    for form in OUT_FORMS:
        for n in (None, 2, 0):
            A(IN16 | INBF | form | 4, n=n, B=0, st=EINVAL)    # one input dtype
        for both in (O16 | OBF, ONHWC | O16 | OBF):
            A(both | 4, B=0, st=EINVAL)
            A(both | 4, n=0, B=0, st=EINVAL)
    for inp in (0, IN16, INBF):
        for form in (O16, OBF, ONHWC | O16, ONHWC | OBF):
            A(inp | form | 4, B=0, out=ODD, st=EINVAL)
            A(inp | form | 4, B=0, out=ODD + 1)
        A(inp | ONHWC | 4, B=0, out=ODD)
    A(-1, st=EINVAL)
    A(-1, n=2, B=0, st=EINVAL)
    A(C=0, st=EINVAL)
    A(div=0.0, st=EINVAL)
    A(div=float("nan"), st=EINVAL)
    A(L=9, hw=(512, 512), st=EINVAL)
    A(L=8, hw=(128, 128), kernel=TILE)
    A(hw=(7, 30), st=EINVAL)
    A(B=65536, st=EINVAL)
    A(B=65535, hw=(4, 8), L=1, kernel=TILE)
    A(C=(1 << 20) + 16, st=EINVAL)
    A(C=1 << 20, kernel=VEC)
    # invalid in two ways
    A(0x400 | 7, st=EINVAL)
    A(0x400 | 4, n=0, st=EINVAL)
    A(O16 | 7, out=ODD, st=EINVAL)
    A(7, C=0, st=EINVAL)
    A(7, n=5, st=EINVAL)
    A(7, div=0.0, st=EINVAL)
    A(7, B=65536, st=EUNSUP)
    A(7, C=(1 << 20) + 16, st=EUNSUP)
    A(7, f1=0, st=EUNSUP)
    A(7, B=0, st=EUNSUP)
    A(B=65536, f1=0, st=EINVAL)
    A(O16 | 4, C=8, f1=0, st=EINVAL)
    return t


TABLE = rows()


def _div(x):
    return "nan" if x != x else repr(float(x))


def _line(fam, r):
    if fam == "P":
        v = (r["dt"], r["B"], r["H"], r["W"], r["L"], r["r"], r["conv"], r["cout"], r["pyr"],
             r["coords"], r["wp"], r["out"])
    elif fam == "V":
        v = (r["B"], r["H"], r["W"], r["L"], r["first"], r["r"], _div(r["div"]), r["vol"],
             r["coords"], r["out"])
    else:
        v = (r["B"], r["H"], r["W"], r["C"], r["L"], r["n"], r["call"], r["r"], _div(r["div"]),
             r["f1"], r["arr"], r["coords"], r["out"], r["ws"], r["wsb"], *r["lv"])
    return fam + " " + " ".join(str(x) for x in v)


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """The planner's answers for TABLE: the sanitized program's output, parsed."""
    spec = importlib.util.spec_from_file_location(
        "_dxr_build_lp", REPO / "optical-flow_dexi-raft_amd" / "build.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    d = tmp_path_factory.mktemp("lookup_plan")
    exe, req = d / "lookup_plan_table", d / "requests.txt"
    subprocess.run([b.hipcc(), "-x", "c++", "-std=c++17", "-O1", "-g",
                    "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover",
                    f"-I{REPO / 'include'}", f"-I{CSRC}",
                    str(REPO / "tests" / "cpp" / "lookup_plan_table.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    req.write_text("".join(_line(fam, r) + "\n" for fam, r, _ in TABLE))
    res = subprocess.run([str(exe), str(req)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    out = []
    for ln in res.stdout.splitlines():
        st, unit, name, rest = ln.split("\t")
        out.append((int(st), unit, name, tuple(int(x) for x in rest.split())))
    assert len(out) == len(TABLE)
    return out


def test_planner_includes_no_hip():
    """The planner and the layout header are host-only: nothing of HIP."""
    for h, allowed in (("lookup_plan.h", ["stdint.h", "dexiraft_corr.h", "pyramid_layout.h"]),
                       ("pyramid_layout.h", ["stdint.h"])):
        incs = re.findall(r'#include\s+[<"]([^>"]+)[>"]', (CSRC / h).read_text())
        assert incs == allowed, (h, incs)
    prog = (REPO / "tests" / "cpp" / "lookup_plan_table.cpp").read_text()
    assert re.findall(r'#include\s+"([^"]+)"', prog) == ["lookup_plan.h"]
    # and the HIP units get the layout through the one header
    assert '#include "pyramid_layout.h"' in (CSRC / "dxr_common.h").read_text()


def test_table_covers_every_row_of_the_header():
    """Every unit and kernel name the rows expect stands in the header's table, and
    the rows reach every (unit, kernel) of each family."""
    table = HEADER.read_text().split("Lookup kernels by request", 1)[1].split("*/", 1)[0]
    for fam, every in (("P", ALL_P), ("V", ALL_V), ("A", ALL_A)):
        for unit, name in every:
            assert unit in table and name in table, (unit, name)
        reached = {(e[1], e[2]) for f, _, e in TABLE if f == fam and e[0] == OK and e[2] != NONE}
        assert reached == every, (fam, every ^ reached)


def test_every_row_of_the_table(planned):
    bad = []
    for i, ((fam, r, exp), got) in enumerate(zip(TABLE, planned)):
        if got[:3] != exp[:3]:
            bad.append((i, _line(fam, r), exp, got))
        elif len(exp) > 3:
            detail = got[3][:-1] if fam == "A" else got[3]
            if detail != exp[3:]:
                bad.append((i, _line(fam, r), exp, got))
    assert not bad, "\n".join(map(str, bad[:40]))


def test_workspace_bytes_through_the_c_abi(planned):
    """dxr_alt_workspace_bytes: the planner's value for every on-the-fly row (they
    share the function) and the documented sizes."""
    from dexiraft_amd import _native as nat
    wsb = nat.load().dxr_alt_workspace_bytes
    for (fam, r, _), got in zip(TABLE, planned):
        if fam == "A":
            want = alt_ws_bytes(r["B"], r["H"], r["W"], r["L"])
            assert got[3][-1] == want == wsb(r["B"], r["H"], r["W"], r["L"]), _line(fam, r)
    assert wsb(1, 55, 128, 4) == 4 * ((20 * 16 * 14 * 32 + 4 * 65 * 4097 + 4 * 64 + 15) & ~15)
    assert wsb(0, 8, 8, 1) == 0 and wsb(-1, 8, 8, 1) == -1 and wsb(1, 8, 8, 9) == -1
    assert wsb(1, 1 << 15, (1 << 15) + 1, 1) == -1


def test_refused_rows_answer_the_same_through_the_c_abi():
    from dexiraft_amd import _native as nat
    lib = nat.load()
    n = {"P": 0, "V": 0, "A": 0}
    for fam, r, exp in TABLE:
        if exp[0] == OK and exp[2] != NONE:
            continue            # would launch
        if fam == "P":
            if r["conv"]:
                got = lib.dxr_corr_lookup_conv1x1(r["pyr"] or None, r["dt"], r["B"], r["H"], r["W"],
                                                  r["L"], r["r"], r["coords"] or None,
                                                  r["wp"] or None, None, r["cout"], 1,
                                                  r["out"] or None, None)
            else:
                got = lib.dxr_corr_lookup(r["pyr"] or None, r["dt"], r["B"], r["H"], r["W"], r["L"],
                                          r["r"], r["coords"] or None, r["out"] or None, None)
        elif fam == "V":
            got = lib.dxr_alt_volume_lookup(r["vol"] or None, r["coords"] or None, r["out"] or None,
                                            r["B"], r["H"], r["W"], r["L"], r["first"], r["r"],
                                            r["div"], None)
        else:
            ptrs = (ctypes.c_void_p * 8)(*r["lv"]) if r["arr"] else None
            head = (r["f1"] or None, ptrs, r["coords"] or None, r["out"] or None, r["B"], r["H"],
                    r["W"], r["C"], r["L"])
            if r["call"]:
                got = lib.dxr_alt_corr_lookup_levels_ws(*head, r["n"], r["r"], r["div"],
                                                        r["ws"] or None, r["wsb"], None)
            elif r["ws"]:
                got = lib.dxr_alt_corr_lookup_ws(*head, r["r"], r["div"], r["ws"], r["wsb"], None)
            else:
                got = lib.dxr_alt_corr_lookup(*head, r["r"], r["div"], None)
        assert got == exp[0], _line(fam, r)
        n[fam] += 1
    assert min(n.values()) > 150, n
    assert lib.dxr_last_hip_error() == 0
