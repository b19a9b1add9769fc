#!/usr/bin/env python3
"""Same-process A/B of the float16 pyramid (DXR_PYR_F16) against the float32 pyramid.

float16 fmaps (what autocast encoders emit), through the C-ABI, one shape per process:

  build    p32  : DXR_F16 fmaps -> float32 pyramid (the default of float16 fmaps)
           p32b : the same arm again (an A/A: the run-to-run spread of the baseline)
           p16  : DXR_F16 fmaps -> float16 pyramid (the same kernel, float16 stores)
  lookup   one radius-4, 4-level lookup from each pyramid, float32 and float16 outputs:
           l32 / l32b (A/A) / l16, and l32h / l32hb (A/A) / l16h (DXR_OUT_F16)

Both fmap layouts are timed for the build (NCHW: 16-bit pack pass + LDS-DMA build;
channels-last: the build alone); the lookup does not depend on the layout.  Before
timing, the float16 pyramid is checked against ``.half()`` of the float32 one (whole
paged buffer, bit for bit) and the lookups against each other (the float16-pyramid
lookup is not expected to equal the float32-pyramid one; its max difference over
max |value| is recorded).  Each arm is captured as a HIP graph (--reps builds, or
--sets lookups over as many coordinate sets) and the graphs are replayed in
interleaved rounds after a clock warm-up (HIP events), as scripts/ab_build_f16.py
and scripts/ab_lookup_out16.py do.  Block memory: torch's peak allocation over one
``CorrBlock(...)`` construction per pyramid dtype, and the pyramid buffers' bytes.
The record carries the box's identity and the calibration of ``bench.py --full``.

Usage: python scripts/ab_build_pyr16.py --shape 1x55x128 --out profiles/.../x.json
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

BUILD_ARMS = ("p32", "p32b", "p16")
LOOKUP_ARMS = ("l32", "l32b", "l16", "l32h", "l32hb", "l16h")


def _time_graphs(graphs, arms, rounds, per, stream):
    res = {v: [] for v in arms}
    for _ in range(10):
        for v in arms:
            graphs[v].replay()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for v in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            graphs[v].replay()
            e1.record(stream)
            torch.cuda.synchronize()
            res[v].append(e0.elapsed_time(e1) * 1e3 / per)
    return res


def _summary(res, base, base_b, new):
    med = {v: float(np.median(x)) for v, x in res.items()}
    spread = abs(med[base_b] - med[base]) / med[base]
    return {
        "us_min_med_max": {v: [round(min(res[v]), 2), round(med[v], 2), round(max(res[v]), 2)]
                           for v in (base, base_b, new)},
        "new_over_base_median": round(med[new] / med[base], 4),
        "base_aa_spread": round(spread, 4),
        "new_faster_beyond_spread": bool(med[base] - med[new] > abs(med[base_b] - med[base])
                                         and max(res[new]) < min(min(res[base]), min(res[base_b]))),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="1x55x128", help="BxHxW (D = 256)")
    ap.add_argument("--layouts", nargs="+", default=["nchw", "nhwc"], choices=["nchw", "nhwc"])
    ap.add_argument("--reps", type=int, default=50, help="builds per graph")
    ap.add_argument("--sets", type=int, default=24, help="lookups (coordinate sets) per graph")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--no-calibration", action="store_true")
    ap.add_argument("--out", default=None, help="write the JSON record here too")
    a = ap.parse_args()
    import bench
    import dexiraft_amd
    from dexiraft_amd import _native as nat
    lib = dexiraft_amd.load_native()
    if not torch.cuda.is_available():
        raise SystemExit("ab_build_pyr16.py needs a HIP device")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    calib = None if a.no_calibration else bench.calibrate(dev, stream)
    D, L, R = 256, 4, 4
    B, H, W = (int(v) for v in a.shape.split("x"))
    div = float(np.sqrt(np.float32(D)))
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    # fnet-like values (tests/datagen.py: N(1.1, 1.45^2)) rounded to float16
    h1 = (1.1 + 1.45 * torch.randn((B, D, H, W), generator=g, device=dev)).half()
    h2 = (1.1 + 1.45 * torch.randn((B, D, H, W), generator=g, device=dev)).half()
    n = lib.dxr_pyramid_numel(B, H, W, L)
    pyr = {"p32": torch.empty(n, device=dev, dtype=torch.float32),
           "p16": torch.empty(n, device=dev, dtype=torch.float16)}
    pyr["p32b"] = pyr["p32"]
    code_of = {"p32": nat.DXR_F32, "p32b": nat.DXR_F32, "p16": nat.DXR_PYR_F16}
    record = {"what": "float16 fmaps: float32 pyramid vs float16 pyramid (DXR_PYR_F16), us per build "
                      "and per lookup (scripts/ab_build_pyr16.py)",
              "shape": [B, D, H, W], "reps": a.reps, "sets": a.sets, "rounds": a.rounds,
              "box": bench.box_identity(dev), "calibration": calib,
              "pyramid_bytes": {"float32": n * 4, "float16": n * 2}, "build": {}}

    # ---- build, per layout
    for layout in a.layouts:
        code = nat.DXR_NCHW if layout == "nchw" else nat.DXR_NHWC
        mf = torch.contiguous_format if layout == "nchw" else torch.channels_last
        f1, f2 = h1.contiguous(memory_format=mf), h2.contiguous(memory_format=mf)
        wsb = 0 if layout == "nhwc" else max(lib.dxr_build_workspace_bytes(nat.DXR_F16, B, D, H, W), 0)
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)

        def build(v):
            st = lib.dxr_corr_pyramid_build_ws(f1.data_ptr(), f2.data_ptr(), nat.DXR_F16, code, B, D,
                                               H, W, L, div, pyr[v].data_ptr(), code_of[v],
                                               nat.DXR_BUILD_AUTO, ws.data_ptr() if wsb else None,
                                               wsb, stream.cuda_stream)
            assert st == 0, (v, layout, st)

        graphs = {}
        with torch.cuda.stream(stream):
            build("p32")
            build("p16")
            torch.cuda.synchronize()
            equal = bool(torch.equal(pyr["p16"].view(torch.int16),
                                     pyr["p32"].half().view(torch.int16)))
            assert equal, f"{layout}: the float16 pyramid is not .half() of the float32 pyramid"
            for v in BUILD_ARMS:
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr, stream=stream):
                    for _ in range(a.reps):
                        build(v)
                graphs[v] = gr
            res = _time_graphs(graphs, BUILD_ARMS, a.rounds, a.reps, stream)
        rec = _summary(res, "p32", "p32b", "p16")
        rec["p16_equals_half_of_p32_bitwise"] = equal
        record["build"][layout] = rec
        del graphs

    # ---- one lookup (both pyramids hold the last layout's build: the same values)
    rd = 2 * R + 1
    gc = torch.Generator(device=dev)
    gc.manual_seed(11)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32),
                            torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    grid = torch.stack([xs, ys])[None].expand(B, 2, H, W)
    coords = [(grid + 4.0 * torch.randn((B, 2, H, W), generator=gc, device=dev)).contiguous()
              for _ in range(a.sets)]
    out32 = torch.empty((B, L * rd * rd, H, W), device=dev, dtype=torch.float32)
    out16 = torch.empty((B, L * rd * rd, H, W), device=dev, dtype=torch.float16)
    arms = {"l32": ("p32", 0, out32), "l32b": ("p32", 0, out32), "l16": ("p16", 0, out32),
            "l32h": ("p32", nat.DXR_OUT_F16, out16), "l32hb": ("p32", nat.DXR_OUT_F16, out16),
            "l16h": ("p16", nat.DXR_OUT_F16, out16)}

    def lookup(v, c):
        p, flag, out = arms[v]
        st = lib.dxr_corr_lookup(pyr[p].data_ptr(), code_of[p] | flag, B, H, W, L, R, c.data_ptr(),
                                 out.data_ptr(), stream.cuda_stream)
        assert st == 0, (v, st)

    graphs = {}
    with torch.cuda.stream(stream):
        lookup("l32", coords[0])
        torch.cuda.synchronize()
        ref = out32.clone()
        lookup("l16", coords[0])
        torch.cuda.synchronize()
        diff = float((out32 - ref).abs().max() / ref.abs().max())
        # and the float16-pyramid lookup is the float32 lookup of the widened cells
        wide = pyr["p16"].float()
        st = lib.dxr_corr_lookup(wide.data_ptr(), nat.DXR_F32, B, H, W, L, R, coords[0].data_ptr(),
                                 ref.data_ptr(), stream.cuda_stream)
        assert st == 0
        torch.cuda.synchronize()
        same = bool(torch.equal(out32, ref))
        assert same, "float16-pyramid lookup != float32 lookup of the widened pyramid"
        del wide, ref
        for v in LOOKUP_ARMS:
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=stream):
                for c in coords:
                    lookup(v, c)
            graphs[v] = gr
        res = _time_graphs(graphs, LOOKUP_ARMS, a.rounds, a.sets, stream)
    record["lookup"] = {
        "radius": R, "levels": L,
        "l16_equals_f32_lookup_of_widened_pyramid": same,
        "l16_vs_l32_max_diff_over_max": diff,
        "out_float32": _summary(res, "l32", "l32b", "l16"),
        "out_float16": _summary(res, "l32h", "l32hb", "l16h"),
    }
    del graphs, pyr, out32, out16, coords

    # ---- block memory: torch's peak over one CorrBlock construction (NCHW fmaps)
    mem = {}
    for name, kw in (("float32", {}), ("float16", {"pyramid_dtype": torch.float16})):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        cb = dexiraft_amd.CorrBlock(h1, h2, **kw)
        torch.cuda.synchronize()
        mem[name] = {"peak_bytes_over_construction": torch.cuda.max_memory_allocated(dev) - base,
                     "held_bytes": torch.cuda.memory_allocated(dev) - base}
        del cb
    record["block_memory"] = mem

    line = json.dumps(record)
    print(line, flush=True)
    if a.out:
        out = Path(a.out)
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(record, indent=1) + "\n")


if __name__ == "__main__":
    main()
