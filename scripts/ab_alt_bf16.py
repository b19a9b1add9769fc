#!/usr/bin/env python3
"""Same-process A/B of AlternateCorrBlock on bfloat16 fmaps (profiles only).

``AlternateCorrBlock.NATIVE_BF16 = False`` (the constructor widens the fmaps and
every call is the parent commit's, bit for bit) against ``True`` (bfloat16
operands in place, ``DXR_ALT_IN_BF16``), on bfloat16 fmaps and bench.py's
coordinate model, in one process after a clock warm-up, arms interleaved.

Arms: ``wide``, ``wide_b`` (the same thing twice: an A/A whose largest difference
within a round is the noise floor) and ``native``.  Per arm:
  lookup        us per lookup: a step graph of ``--iters`` lookups (12) of one
                block, divided by ``--iters``
  construct     us per block construction (a graph of one constructor)
  peak_extra    torch.cuda.max_memory_allocated above the inputs over one
                eager construction + ``--iters`` lookups (outputs included)
The native outputs are compared with the widened ones before anything is
timed: the two sum the same exact products through different instructions, so
they are not bit-equal; the largest difference must stay below 1e-5 of the
largest output (a sanity check — tests/test_gpu_alt_bf16.py holds the per-output
criterion) and is recorded.  Not measured: the kernel's time alone under a
profiler.

Usage (each GPU step under its own time limit):
  timeout -k 10 300 python scripts/ab_alt_bf16.py --workload 1080p --out profiles/.../x.json
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

SHAPES = {"sintel": (55, 128), "1080p": (136, 240)}
ARMS = ("wide", "wide_b", "native")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="1080p", choices=sorted(SHAPES))
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--iters", type=int, default=12, help="lookups per step")
    ap.add_argument("--reps", type=int, default=10, help="graph replays per timed round")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--no-calibration", action="store_true")
    ap.add_argument("--out", default=None, help="write the JSON record here too")
    a = ap.parse_args()
    import bench
    import dexiraft_amd
    dexiraft_amd.load_native()
    if not torch.cuda.is_available():
        raise SystemExit("ab_alt_bf16.py needs a HIP device")
    Block = dexiraft_amd.AlternateCorrBlock
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    calib = None if a.no_calibration else bench.calibrate(dev, stream)
    B, (H, W), D, L, r = a.batch, SHAPES[a.workload], 256, 4, 4
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    f1 = torch.randn((B, D, H, W), generator=g, device=dev).bfloat16()
    f2 = torch.randn((B, D, H, W), generator=g, device=dev).bfloat16()
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32),
                            torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    grid = torch.stack((xs, ys))[None].expand(B, 2, H, W)
    coords = [(grid + 4.0 * torch.randn((B, 2, H, W), generator=g, device=dev)).contiguous()
              for _ in range(a.iters)]

    def make(arm):
        default = Block.NATIVE_BF16
        Block.NATIVE_BF16 = arm == "native"
        try:
            return Block(f1, f2, num_levels=L, radius=r)
        finally:
            Block.NATIVE_BF16 = default

    with torch.no_grad(), torch.cuda.stream(stream):
        blocks = {v: make(v) for v in ARMS}
        assert blocks["native"]._inbf16 and not blocks["wide"]._inbf16
        assert blocks["native"]._f1_nhwc.dtype == torch.bfloat16
        assert blocks["wide"]._f1_nhwc.dtype == torch.float32
        first = blocks["native"].coarse_first_level
        want = [blocks["wide"](c) for c in coords]
        got = [blocks["native"](c) for c in coords]
        torch.cuda.synchronize()
        assert blocks["native"]._inbf16, "the library declined the flag"
        diff = max(float((x - y).abs().max()) for x, y in zip(got, want))
        scale = max(float(y.abs().max()) for y in want)
        assert diff <= 1e-5 * scale, f"native differs from widened by {diff} (largest output {scale})"
        del want, got

        # peak memory of one eager construction + step, above the inputs
        peak = {}
        for v in ARMS:
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            blk = make(v)
            keep = [blk(c) for c in coords]
            torch.cuda.synchronize()
            peak[v] = torch.cuda.max_memory_allocated(dev) - base
            del blk, keep

        look, cons = {}, {}
        for v in ARMS:
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=stream):
                keep = [blocks[v](c) for c in coords]
            look[v] = (gr, keep)
            gc = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gc, stream=stream):
                kb = make(v)
            cons[v] = (gc, kb)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.5:   # clock warm-up
            for v in ARMS:
                look[v][0].replay()
                cons[v][0].replay()
            torch.cuda.synchronize()

        def timed(graph, per):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.reps):
                graph.replay()
            e1.record(stream)
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / a.reps / per

        res_l, res_c = {v: [] for v in ARMS}, {v: [] for v in ARMS}
        for _ in range(a.rounds):
            for v in ARMS:
                res_l[v].append(timed(look[v][0], a.iters))
            for v in ARMS:
                res_c[v].append(timed(cons[v][0], 1))
    med_l = {v: float(np.median(x)) for v, x in res_l.items()}
    med_c = {v: float(np.median(x)) for v, x in res_c.items()}
    # the noise floor: the largest difference of the two identical arms within one round
    spread_l = max(abs(x - y) for x, y in zip(res_l["wide"], res_l["wide_b"]))
    spread_c = max(abs(x - y) for x, y in zip(res_c["wide"], res_c["wide_b"]))
    mmm = lambda res: {v: [round(min(x), 2), round(float(np.median(x)), 2), round(max(x), 2)]
                       for v, x in res.items()}
    record = {
        "what": "AlternateCorrBlock on bfloat16 fmaps, NATIVE_BF16 False (wide, wide_b) against "
                "True (native), scripts/ab_alt_bf16.py",
        "workload": a.workload, "shape": [B, D, H, W], "radius": r, "num_levels": L,
        "coarse_first_level": first, "iters": a.iters, "reps": a.reps, "rounds": a.rounds,
        "box": bench.box_identity(dev), "calibration": calib,
        "native_minus_widened_max_abs": diff, "largest_widened_output": scale,
        "lookup_us_min_med_max": mmm(res_l),
        "construct_us_min_med_max": mmm(res_c),
        "lookup_aa_spread_us": round(spread_l, 3),
        "construct_aa_spread_us": round(spread_c, 3),
        "aa_spread_what": "max over rounds of |wide - wide_b| within a round",
        "lookup_native_minus_wide_us": round(med_l["native"] - med_l["wide"], 3),
        "lookup_native_over_wide": round(med_l["native"] / med_l["wide"], 4),
        "construct_native_over_wide": round(med_c["native"] / med_c["wide"], 4),
        "native_faster_than_wide_by_more_than_aa_spread": bool(
            min(med_l["wide"], med_l["wide_b"]) - med_l["native"] > spread_l),
        "peak_extra_bytes": peak,
        "peak_extra_what": "max_memory_allocated above the inputs: one eager construction + "
                           "--iters lookups, all outputs alive",
    }
    print(json.dumps(record), flush=True)
    if a.out:
        out = Path(a.out)
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(record, indent=1) + "\n")


if __name__ == "__main__":
    main()
