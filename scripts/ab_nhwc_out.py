#!/usr/bin/env python3
"""Same-process A/B of channels-last lookup outputs inside the step (profiles only).

What a channels-last update block pays for the lookup tensor, measured where it
is paid: in the step (the build and then 12 lookups on 12 coordinate sets,
bench.py's; isolated back-to-back lookups mislead), one HIP graph
per arm, interleaved rounds in one process after a clock warm-up.

Arms:
  nchw, nchw_b   the NCHW lookups, twice: an A/A whose spread is the noise floor
  nchw_copy      NCHW lookups, each followed by
                 ``.contiguous(memory_format=torch.channels_last)``: what a
                 channels-last consumer pays without the feature (the baseline)
  cl_wt, cl_nt, cl_plain
                 the kernels' own channels-last stores with the store policy forced
                 (write-through / non-temporal / plain: ``dxr_xp_lookup_nhwc`` of the
                 experiments target, ``build.py --experiments``)
  cl             the product call (``memory_format=torch.channels_last``): the
                 policy ``launch_lookup_nhwc_r`` chooses
``--conv``: the same for ``lookup_conv1x1`` (324 -> 256, bias, ReLU; 12 calls, no
build in the step; policies non-temporal / plain — its 16- and 8-byte vector stores
have no write-through form).

Every channels-last arm's outputs are checked bit for bit against the NCHW arm's
before anything is timed.  The record carries the box's identity and the
calibration of ``bench.py --full``.

Usage: python scripts/ab_nhwc_out.py --workload sintel --batch 8 --out profiles/.../x.json
       python scripts/ab_nhwc_out.py --workload kitti --batch 8 --fmap bf16
       python scripts/ab_nhwc_out.py --workload sintel --batch 8 --out-dtype f16
       python scripts/ab_nhwc_out.py --workload sintel --batch 2 --conv
"""
from __future__ import annotations

import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

SHAPES = {"sintel": (55, 128), "chairs": (46, 62), "kitti": (47, 156), "1080p": (136, 240)}
FMAP = {"f32": torch.float32, "bf16": torch.bfloat16}
POLICY = {"cl_wt": 0, "cl_nt": 1, "cl_plain": 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="sintel", choices=sorted(SHAPES))
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--fmap", default="f32", choices=sorted(FMAP))
    ap.add_argument("--out-dtype", default="f32", choices=["f32", "f16"])
    ap.add_argument("--conv", action="store_true", help="time lookup_conv1x1 (324 -> 256)")
    ap.add_argument("--iters", type=int, default=12, help="lookups per step")
    ap.add_argument("--reps", type=int, default=20, help="graph replays per timed round")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--no-calibration", action="store_true")
    ap.add_argument("--out", default=None, help="write the JSON record here too")
    a = ap.parse_args()
    import bench
    import dexiraft_amd
    from dexiraft_amd import _native as nat
    dexiraft_amd.load_native()
    if not torch.cuda.is_available():
        raise SystemExit("ab_nhwc_out.py needs a HIP device")
    xp = ctypes.CDLL(str(nat.LIB_PATH.with_name("libdexiraft_corr_exp.so")))
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    xp.dxr_xp_lookup_nhwc.restype = i32
    xp.dxr_xp_lookup_nhwc.argtypes = [vp, i32, i32, i64, i64, i64, i32, vp, vp, vp, i64, vp, i32, vp]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    calib = None if a.no_calibration else bench.calibrate(dev, stream)
    B, (H, W), D = a.batch, SHAPES[a.workload], 256
    odt = None if a.out_dtype == "f32" else torch.float16
    oflag = 0 if odt is None else nat.DXR_OUT_F16
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    f1 = torch.randn((B, D, H, W), generator=g, device=dev).to(FMAP[a.fmap])
    f2 = torch.randn((B, D, H, W), generator=g, device=dev).to(FMAP[a.fmap])
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32),
                            torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    grid = torch.stack((xs, ys))[None].expand(B, 2, H, W)
    coords = [(grid + 4.0 * torch.randn((B, 2, H, W), generator=g, device=dev)).contiguous()
              for _ in range(a.iters)]
    wt = bias = planes = None
    cout = 0
    if a.conv:
        from dexiraft_amd.corr import _packed_weight
        cout = 256
        wt = torch.randn((cout, 324), generator=g, device=dev) / 18.0
        bias = 0.5 * torch.randn((cout,), generator=g, device=dev)
        planes = _packed_weight(wt, dev)
    arms = ["nchw", "nchw_b", "nchw_copy"] + (["cl_nt", "cl_plain"] if a.conv else list(POLICY)) + ["cl"]
    C = cout if a.conv else 324

    with torch.no_grad(), torch.cuda.stream(stream):
        cb = dexiraft_amd.CorrBlock(f1, f2, num_levels=4, radius=4)

        def lookup(arm, c):
            if arm in POLICY:
                o = torch.empty((B, C, H, W), dtype=odt or torch.float32, device=dev,
                                memory_format=torch.channels_last)
                st = xp.dxr_xp_lookup_nhwc(cb._buf.data_ptr(), cb._pyr_dt, oflag, B, H, W, 4,
                                           c.data_ptr(), nat.ptr(planes), nat.ptr(bias), cout,
                                           o.data_ptr(), POLICY[arm], stream.cuda_stream)
                assert st == 0, st
                return o
            fmt = torch.channels_last if arm == "cl" else None
            if a.conv:
                o = cb.lookup_conv1x1(c, wt, bias, out_dtype=odt, memory_format=fmt)
            else:
                o = cb(c, out_dtype=odt, memory_format=fmt)
            return o.contiguous(memory_format=torch.channels_last) if arm == "nchw_copy" else o

        def step(arm):
            if not a.conv:
                _, _, st = cb._launch_build(f1, f2)
                assert st == 0
            return [lookup(arm, c) for c in coords]   # every output alive: no reuse inside the graph

        ref = step("nchw")
        torch.cuda.synchronize()
        bits = torch.int32 if odt is None else torch.int16
        for arm in arms[2:]:
            got = step(arm)
            torch.cuda.synchronize()
            for x, y in zip(got, ref):
                assert x.is_contiguous(memory_format=torch.channels_last), arm
                assert torch.equal(x.contiguous().view(bits), y.view(bits)), arm
            del got
        out_bytes = ref[0].numel() * ref[0].element_size()
        del ref
        graphs, res = {}, {v: [] for v in arms}
        for v in arms:
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=stream):
                keep = step(v)
            graphs[v] = (gr, keep)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.5:   # clock warm-up
            for v in arms:
                graphs[v][0].replay()
            torch.cuda.synchronize()
        for _ in range(a.rounds):
            for v in arms:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.reps):
                    graphs[v][0].replay()
                e1.record(stream)
                torch.cuda.synchronize()
                res[v].append(e0.elapsed_time(e1) * 1e3 / a.reps)
    med = {v: float(np.median(x)) for v, x in res.items()}
    spread = abs(med["nchw_b"] - med["nchw"])
    record = {
        "what": "us per step graph (build + 12 lookups; --conv: 12 lookup_conv1x1), "
                "scripts/ab_nhwc_out.py",
        "op": "lookup_conv1x1 324->256" if a.conv else "build + lookups",
        "workload": a.workload, "shape": [B, D, H, W], "fmap": a.fmap,
        "pyramid": str(cb._buf.dtype)[6:], "out_dtype": a.out_dtype, "out_bytes_per_lookup": out_bytes,
        "iters": a.iters, "reps": a.reps, "rounds": a.rounds,
        "box": bench.box_identity(dev), "calibration": calib,
        "channels_last_equals_nchw_bitwise": True,
        "us_per_step_min_med_max": {v: [round(min(x), 1), round(med[v], 1), round(max(x), 1)]
                                    for v, x in res.items()},
        "aa_spread_us": round(spread, 2),
        "aa_spread_rel": round(spread / med["nchw"], 4),
        "over_nchw_copy_median": {v: round(med[v] / med["nchw_copy"], 4) for v in arms[3:]},
        "over_nchw_median": {v: round(med[v] / med["nchw"], 4) for v in arms[2:]},
        # the expectation of the A/B: the product's channels-last call beats lookup + copy
        "cl_below_nchw_copy_beyond_spread": bool(med["nchw_copy"] - med["cl"] > spread),
    }
    print(json.dumps(record), flush=True)
    if a.out:
        out = Path(a.out)
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(record, indent=1) + "\n")


if __name__ == "__main__":
    main()
