#!/usr/bin/env python3
"""Same-process A/B of AlternateCorrBlock's coarse volumes in float16 (profiles only).

``AlternateCorrBlock(..., volume_dtype=torch.float16)`` (the volume GEMM stores
float16 cells, ``DXR_ALT_VOL_F16``; the volume lookup widens them on load)
against the default float32 volumes, on bench.py's coordinate model, in one
process after a clock warm-up, arms interleaved.

Arms: ``vol32``, ``vol32_b`` (the same thing twice: an A/A whose largest
difference within a round is the noise floor) and ``vol16``.  Per arm:
  lookup        us per lookup: a step graph of ``--iters`` lookups (12) of one
                block, divided by ``--iters``
  construct     us per block construction (a graph of one constructor)
  peak_extra    torch.cuda.max_memory_allocated above the inputs over one
                eager construction + ``--iters`` lookups (outputs included)
Before anything is timed the two bit-equalities of the option's definition are
checked: the float16 buffer is the float32 buffer's ``.half()``, and every
float16-volume lookup equals that of a float32-volume block whose volumes are
``.half().float()`` of themselves.

Usage: python scripts/ab_alt_vol16.py --batch 1 --fmaps float32
       (writes profiles/r16/alt_vol16/<workload>_b<B>_<fmaps>.json unless --out is given)
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
ARMS = ("vol32", "vol32_b", "vol16")


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="1080p", choices=sorted(SHAPES))
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--fmaps", default="float32", choices=("float32", "float16"))
    ap.add_argument("--iters", type=int, default=12, help="lookups per step")
    ap.add_argument("--reps", type=int, default=10, help="graph replays per timed round")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--no-calibration", action="store_true")
    ap.add_argument("--out", default=None, help="the JSON record's path")
    a = ap.parse_args()
    import bench
    import dexiraft_amd
    dexiraft_amd.load_native()
    if not torch.cuda.is_available():
        raise SystemExit("ab_alt_vol16.py needs a HIP device")
    Block = dexiraft_amd.AlternateCorrBlock
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    calib = None if a.no_calibration else bench.calibrate(dev, stream)
    B, (H, W), D, L, r = a.batch, SHAPES[a.workload], 256, 4, 4
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    fdt = getattr(torch, a.fmaps)
    f1 = torch.randn((B, D, H, W), generator=g, device=dev).to(fdt)
    f2 = torch.randn((B, D, H, W), generator=g, device=dev).to(fdt)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32),
                            torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    grid = torch.stack((xs, ys))[None].expand(B, 2, H, W)
    coords = [(grid + 4.0 * torch.randn((B, 2, H, W), generator=g, device=dev)).contiguous()
              for _ in range(a.iters)]

    def make(arm):
        return Block(f1, f2, num_levels=L, radius=r,
                     volume_dtype=torch.float16 if arm == "vol16" else None)

    with torch.no_grad(), torch.cuda.stream(stream):
        blocks = {v: make(v) for v in ARMS}
        firsts = {v: blocks[v].coarse_first_level for v in ARMS}
        dtypes = {v: str(blocks[v].volume_dtype) for v in ARMS}
        v16, v32 = blocks["vol16"]._volumes, blocks["vol32"]._volumes
        buffer_equal = lookups_equal = None
        if v16 is not None and v32 is not None and firsts["vol16"] == firsts["vol32"]:
            assert v16.dtype == torch.float16 and v32.dtype == torch.float32
            assert v16.numel() == v32.numel()
            buffer_equal = bool(torch.equal(_bits(v16), _bits(v32.half())))
            assert buffer_equal, "the float16 buffer is not the float32 buffer's .half()"
            ref = make("vol32")
            ref._volumes = ref._volumes.half().float()
            lookups_equal = True
            for c in coords:
                x, y = blocks["vol16"](c), ref(c)
                lookups_equal &= bool(torch.equal(_bits(x), _bits(y)))
            assert lookups_equal, "a float16-volume lookup differs from the widened volume's"
            del ref
        torch.cuda.synchronize()

        # peak memory of one eager construction + step, above the inputs
        peak, held = {}, {}
        for v in ARMS:
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            blk = make(v)
            torch.cuda.synchronize()
            held[v] = torch.cuda.memory_allocated(dev) - base
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
    spread_l = max(abs(x - y) for x, y in zip(res_l["vol32"], res_l["vol32_b"]))
    spread_c = max(abs(x - y) for x, y in zip(res_c["vol32"], res_c["vol32_b"]))
    mmm = lambda res: {v: [round(min(x), 2), round(float(np.median(x)), 2), round(max(x), 2)]
                       for v, x in res.items()}
    record = {
        "what": "AlternateCorrBlock coarse volumes, float32 (vol32, vol32_b) against "
                "volume_dtype=torch.float16 (vol16), scripts/ab_alt_vol16.py",
        "workload": a.workload, "shape": [B, D, H, W], "fmaps": a.fmaps, "radius": r,
        "num_levels": L, "coarse_first_level": firsts, "volume_dtype": dtypes,
        "volume_numel": {v: (None if blocks[v]._volumes is None else blocks[v]._volumes.numel())
                         for v in ARMS},
        "iters": a.iters, "reps": a.reps, "rounds": a.rounds,
        "box": bench.box_identity(dev), "calibration": calib,
        "buffer_equals_float32_half": buffer_equal,
        "lookups_equal_widened_volume": lookups_equal,
        "lookup_us_min_med_max": mmm(res_l),
        "construct_us_min_med_max": mmm(res_c),
        "lookup_aa_spread_us": round(spread_l, 3),
        "construct_aa_spread_us": round(spread_c, 3),
        "aa_spread_what": "max over rounds of |vol32 - vol32_b| within a round",
        "lookup_vol16_over_vol32": round(med_l["vol16"] / med_l["vol32"], 4),
        "construct_vol16_over_vol32": round(med_c["vol16"] / med_c["vol32"], 4),
        "held_bytes_after_construction": held,
        "peak_extra_bytes": peak,
        "peak_extra_what": "max_memory_allocated above the inputs: one eager construction + "
                           "--iters lookups, all outputs alive",
    }
    print(json.dumps(record), flush=True)
    out = Path(a.out) if a.out else (REPO / "profiles" / "r16" / "alt_vol16" /
                                     f"{a.workload}_b{B}_{a.fmaps}.json")
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(record, indent=1) + "\n")


if __name__ == "__main__":
    main()
