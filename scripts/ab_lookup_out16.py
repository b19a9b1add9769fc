#!/usr/bin/env python3
"""Same-process A/B of the 16-bit lookup output against the float32 lookup + cast.

What a mixed-precision update block (autocast, core/update.py:90) gets per lookup,
on one CorrBlock and a fixed set of coordinates:

  f32cast  : float32 lookup, then ``.to(dtype)`` — what such a user runs without
             ``out_dtype`` (the cast is autocast's, before convc1)
  f32castb : the same arm again (an A/A: the run-to-run spread of that arm)
  f32      : the float32 lookup alone
  out16    : ``cb(coords, out_dtype=dtype)``: the lookup stores 16-bit values itself

``--conv`` times the same three forms of ``lookup_conv1x1`` (convc1 of the basic
motion encoder, 324 -> 256) instead.  Before timing, out16 is checked bit-equal to
f32cast.  Each arm is captured as a HIP graph of --reps lookups over --reps
coordinate sets and the graphs are replayed in interleaved rounds after a clock
warm-up (HIP events), the way scripts/ab_build_f16.py times builds; one process
per shape.  The record carries the box's identity and the calibration of
``bench.py --full``.

Usage: python scripts/ab_lookup_out16.py --shape 1x55x128 --out profiles/.../x.json
       python scripts/ab_lookup_out16.py --shape 8x47x156 --fmap bf16 --dtype bf16
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

ARMS = ("f32cast", "f32castb", "f32", "out16")
DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="1x55x128", help="BxHxW (D = 256)")
    ap.add_argument("--fmap", default="f32", choices=["f32", "f16", "bf16"],
                    help="fmap dtype (bf16 builds a bf16 pyramid)")
    ap.add_argument("--dtype", default="f16", choices=["f16", "bf16"], help="16-bit output dtype")
    ap.add_argument("--conv", action="store_true", help="time lookup_conv1x1 (324 -> 256)")
    ap.add_argument("--reps", type=int, default=24, help="lookups per graph")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--no-calibration", action="store_true")
    ap.add_argument("--out", default=None, help="write the JSON record here too")
    a = ap.parse_args()
    import bench
    import dexiraft_amd
    dexiraft_amd.load_native()
    if not torch.cuda.is_available():
        raise SystemExit("ab_lookup_out16.py needs a HIP device")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    calib = None if a.no_calibration else bench.calibrate(dev, stream)
    D = 256
    B, H, W = (int(v) for v in a.shape.split("x"))
    dt = DT[a.dtype]
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    # fnet-like fmaps (tests/datagen.py: N(1.1, 1.45^2)); coords = grid + N(0, 4^2),
    # the benchmark's flow model, a fresh set per lookup of the graph
    f1 = (1.1 + 1.45 * torch.randn((B, D, H, W), generator=g, device=dev)).to(DT[a.fmap])
    f2 = (1.1 + 1.45 * torch.randn((B, D, H, W), generator=g, device=dev)).to(DT[a.fmap])
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32),
                            torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    grid = torch.stack([xs, ys])[None].expand(B, 2, H, W)
    coords = [(grid + 4.0 * torch.randn((B, 2, H, W), generator=g, device=dev)).contiguous()
              for _ in range(a.reps)]
    wt = bias = None
    if a.conv:
        wt = torch.randn((256, 324), generator=g, device=dev) / 18.0
        bias = 0.5 * torch.randn((256,), generator=g, device=dev)

    with torch.no_grad(), torch.cuda.stream(stream):
        cb = dexiraft_amd.CorrBlock(f1, f2, num_levels=4, radius=4)

        def run(arm, c):
            if a.conv:
                if arm == "out16":
                    return cb.lookup_conv1x1(c, wt, bias, out_dtype=dt)
                o = cb.lookup_conv1x1(c, wt, bias)
            else:
                if arm == "out16":
                    return cb(c, out_dtype=dt)
                o = cb(c)
            return o if arm == "f32" else o.to(dt)

        ref, got = run("f32cast", coords[0]), run("out16", coords[0])
        torch.cuda.synchronize()
        nan = torch.isnan(ref)
        equal = bool(torch.equal(torch.isnan(got), nan)
                     and torch.equal(got.view(torch.int16)[~nan], ref.view(torch.int16)[~nan]))
        assert equal, "out16 differs from the float32 lookup's cast"
        out_elems = ref.numel()
        del ref, got
        graphs, res = {}, {v: [] for v in ARMS}
        for v in ARMS:
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=stream):
                keep = [run(v, c) for c in coords]   # every output alive: no reuse inside the graph
            graphs[v] = (gr, keep)
        for _ in range(10):
            for v in ARMS:
                graphs[v][0].replay()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for v in ARMS:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                graphs[v][0].replay()
                e1.record(stream)
                torch.cuda.synchronize()
                res[v].append(e0.elapsed_time(e1) * 1e3 / a.reps)
    med = {v: float(np.median(x)) for v, x in res.items()}
    spread = abs(med["f32castb"] - med["f32cast"])
    record = {
        "what": "us per lookup: float32 lookup + cast vs float32 lookup vs 16-bit-output lookup "
                "(scripts/ab_lookup_out16.py)",
        "op": "lookup_conv1x1 324->256" if a.conv else "lookup",
        "shape": [B, D, H, W], "fmap": a.fmap, "pyramid": str(cb._buf.dtype)[6:], "out_dtype": a.dtype,
        "out_elements": out_elems, "reps": a.reps, "rounds": a.rounds,
        "box": bench.box_identity(dev), "calibration": calib,
        "out16_equals_cast_bitwise": equal,
        "us_per_lookup_min_med_max": {v: [round(min(x), 2), round(med[v], 2), round(max(x), 2)]
                                      for v, x in res.items()},
        "aa_spread_us": round(spread, 3),
        "aa_spread_rel": round(spread / med["f32cast"], 4),
        "out16_over_f32cast_median": round(med["out16"] / med["f32cast"], 4),
        "out16_over_f32_median": round(med["out16"] / med["f32"], 4),
        # the two expectations of the A/B
        "out16_below_f32cast_beyond_spread": bool(med["f32cast"] - med["out16"] > spread),
        "out16_not_above_f32_beyond_spread": bool(med["out16"] - med["f32"] <= spread),
    }
    print(json.dumps(record), flush=True)
    if a.out:
        out = Path(a.out)
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(record, indent=1) + "\n")


if __name__ == "__main__":
    main()
