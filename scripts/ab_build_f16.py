#!/usr/bin/env python3
"""Same-process A/B of the float16 build against the f32 build on the same values.

What a mixed-precision user gets with and without the float16 input mode, through
the C-ABI (build only, no lookups), on float16-representable fmaps:

  f32  : the values as float32 -> dxr_corr_pyramid_build_ws (split pass + LDS-DMA
         build, three f16 MFMA products per f32 product): the path behind
         ``CorrBlock(fmap.float())``
  f32b : the same arm again (an A/A: the run-to-run spread of the f32 arm)
  f16  : the values as float16 -> DXR_F16 (NCHW: 16-bit pack pass + LDS-DMA build on
         f16 records; channels-last: the build alone, records read in place)

Both layouts are timed.  Before timing, the f16 pyramid is checked against the
f32 arm's (bit-equal, or within 2e-6 of max as a fallback that is reported).
Each arm is captured as a HIP graph of --reps back-to-back builds and the graphs
are replayed in interleaved rounds after a clock warm-up (HIP events), the way
scripts/ab_build.py times builds.  The record carries the box's identity and the
calibration of ``bench.py --full``.  Run it under ``rocprofv3 --kernel-trace
--stats`` (with small --reps / --rounds) for per-kernel durations.

Usage: python scripts/ab_build_f16.py --shape 1x55x128 --out profiles/.../x.json
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

ARMS = ("f32", "f32b", "f16")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="1x55x128", help="BxHxW (D = 256)")
    ap.add_argument("--layouts", nargs="+", default=["nchw", "nhwc"], choices=["nchw", "nhwc"])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--no-calibration", action="store_true")
    ap.add_argument("--out", default=None, help="write the JSON record here too")
    a = ap.parse_args()
    import bench
    import dexiraft_amd
    from dexiraft_amd import _native as nat
    lib = dexiraft_amd.load_native()
    if not torch.cuda.is_available():
        raise SystemExit("ab_build_f16.py needs a HIP device")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    calib = None if a.no_calibration else bench.calibrate(dev, stream)
    D = 256
    B, H, W = (int(v) for v in a.shape.split("x"))
    div = float(np.sqrt(np.float32(D)))
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    # fnet-like values (tests/datagen.py: N(1.1, 1.45^2)) rounded to float16
    h1 = (1.1 + 1.45 * torch.randn((B, D, H, W), generator=g, device=dev)).half()
    h2 = (1.1 + 1.45 * torch.randn((B, D, H, W), generator=g, device=dev)).half()
    n = lib.dxr_pyramid_numel(B, H, W, 4)
    pyr = torch.empty(n, device=dev, dtype=torch.float32)
    record = {"what": "us per build, f32 build vs f16 build on the same float16-representable "
                      "values (scripts/ab_build_f16.py)",
              "shape": [B, D, H, W], "reps": a.reps, "rounds": a.rounds,
              "box": bench.box_identity(dev), "calibration": calib, "layouts": {}}
    for layout in a.layouts:
        code = nat.DXR_NCHW if layout == "nchw" else nat.DXR_NHWC
        mf = torch.contiguous_format if layout == "nchw" else torch.channels_last
        ops = {"f16": (h1.contiguous(memory_format=mf), h2.contiguous(memory_format=mf), nat.DXR_F16),
               "f32": (h1.float().contiguous(memory_format=mf),
                       h2.float().contiguous(memory_format=mf), nat.DXR_F32)}
        ops["f32b"] = ops["f32"]
        wsb = {k: max(lib.dxr_build_workspace_bytes(v[2], B, D, H, W), 0) for k, v in ops.items()}
        if layout == "nhwc":
            wsb["f16"] = 0   # records read in place
        ws = torch.empty(max(max(wsb.values()), 16), dtype=torch.uint8, device=dev)

        def build(v):
            f1, f2, dt = ops[v]
            st = lib.dxr_corr_pyramid_build_ws(f1.data_ptr(), f2.data_ptr(), dt, code, B, D, H, W,
                                               4, div, pyr.data_ptr(), nat.DXR_F32,
                                               nat.DXR_BUILD_AUTO, ws.data_ptr() if wsb[v] else None,
                                               wsb[v], stream.cuda_stream)
            assert st == 0, (v, layout, st)

        graphs, res = {}, {v: [] for v in ARMS}
        with torch.cuda.stream(stream):
            build("f32")
            torch.cuda.synchronize()
            ref = pyr.clone()
            build("f16")
            torch.cuda.synchronize()
            equal = bool(torch.equal(pyr, ref))
            rel = float((pyr - ref).abs().max() / ref.abs().max())
            assert equal or rel <= 2e-6, (layout, rel)
            del ref
            for v in ARMS:
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr, stream=stream):
                    for _ in range(a.reps):
                        build(v)
                graphs[v] = gr
            for _ in range(10):
                for v in ARMS:
                    graphs[v].replay()
            torch.cuda.synchronize()
            for _ in range(a.rounds):
                for v in ARMS:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    graphs[v].replay()
                    e1.record(stream)
                    torch.cuda.synchronize()
                    res[v].append(e0.elapsed_time(e1) * 1e3 / a.reps)
        med = {v: float(np.median(x)) for v, x in res.items()}
        record["layouts"][layout] = {
            "f16_equals_f32_bitwise": equal, "max_rel_diff": rel,
            "us_per_build_min_med_max": {v: [round(min(x), 2), round(med[v], 2), round(max(x), 2)]
                                         for v, x in res.items()},
            "f16_over_f32_median": round(med["f16"] / med["f32"], 4),
            "f32_aa_spread": round(abs(med["f32b"] - med["f32"]) / med["f32"], 4),
            "f16_faster_beyond_spread": bool(med["f32"] - med["f16"] > abs(med["f32b"] - med["f32"])
                                             and max(res["f16"]) < min(min(res["f32"]),
                                                                       min(res["f32b"]))),
        }
        del graphs
    line = json.dumps(record)
    print(line, flush=True)
    if a.out:
        out = Path(a.out)
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(record, indent=1) + "\n")


if __name__ == "__main__":
    main()
