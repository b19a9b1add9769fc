#!/usr/bin/env python3
"""Same-process A/B of the alternate block's flagged lookup outputs (profiles only).

What a mixed-precision and / or channels-last update block pays for the
on-the-fly lookup tensor: a step of ``--iters`` lookups (12, on 12 coordinate
sets, bench.py's) of one ``AlternateCorrBlock`` — at 1080p the product path,
fine levels on the fly and coarse levels from their volumes — one HIP graph per
arm, interleaved rounds in one process after a clock warm-up.

Arms:
  f32, f32_b      the default float32 NCHW lookups, twice: an A/A whose largest
                  difference within a round is the noise floor
  prev            the same calls through ``--prev-lib`` (the parent commit's
                  library): the default path must stay within the A/A spread
  base_<kind>     float32 NCHW lookups, each followed by ``.to(dtype)`` and / or
                  ``.contiguous(memory_format=torch.channels_last)``: what the
                  consumer pays without the feature
  flag_<kind>     ``AlternateCorrBlock(..., out_dtype=, memory_format=)``: the
                  kernels' own stores
with <kind> in f16, bf16, cl, cl_f16, cl_bf16.  Every flag arm's outputs are
checked bit for bit against its base arm's before anything is timed.

``--only ARM --eager N``: no timing; N eager steps of one arm, for a counter pass
of its own (``rocprofv3 --pmc WRITE_SIZE -- python scripts/ab_alt_out.py ...``;
scripts/pmc_summary.py sums the kernels' counters).

Usage: python scripts/ab_alt_out.py --workload 1080p --out profiles/.../x.json
       python scripts/ab_alt_out.py --workload sintel --prev-lib scripts/libdexiraft_corr_head.so
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

SHAPES = {"sintel": (55, 128), "chairs": (46, 62), "kitti": (47, 156), "1080p": (135, 240)}
CL = torch.channels_last
KINDS = {"f16": (torch.float16, None), "bf16": (torch.bfloat16, None), "cl": (None, CL),
         "cl_f16": (torch.float16, CL), "cl_bf16": (torch.bfloat16, CL)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="1080p", choices=sorted(SHAPES))
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--iters", type=int, default=12, help="lookups per step")
    ap.add_argument("--reps", type=int, default=10, help="graph replays per timed round")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--prev-lib", default=None, help="the parent commit's library (arm `prev`)")
    ap.add_argument("--only", default=None, help="with --eager: the one arm to run")
    ap.add_argument("--eager", type=int, default=0, help="eager steps of --only, no timing")
    ap.add_argument("--no-calibration", action="store_true")
    ap.add_argument("--out", default=None, help="write the JSON record here too")
    a = ap.parse_args()
    import bench
    import dexiraft_amd
    from dexiraft_amd import _native as nat
    from dexiraft_amd.corr import _sqrt_dim
    dexiraft_amd.load_native()
    if not torch.cuda.is_available():
        raise SystemExit("ab_alt_out.py needs a HIP device")
    prev = None
    if a.prev_lib:
        prev = ctypes.CDLL(a.prev_lib)
        for name, (res, args) in nat.SIGNATURES.items():
            if hasattr(prev, name):
                getattr(prev, name).restype = res
                getattr(prev, name).argtypes = args
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    calib = None if (a.no_calibration or a.eager) else bench.calibrate(dev, stream)
    B, (H, W), D, L, r = a.batch, SHAPES[a.workload], 256, 4, 4
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    f1 = torch.randn((B, D, H, W), generator=g, device=dev)
    f2 = torch.randn((B, D, H, W), generator=g, device=dev)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32),
                            torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    grid = torch.stack((xs, ys))[None].expand(B, 2, H, W)
    coords = [(grid + 4.0 * torch.randn((B, 2, H, W), generator=g, device=dev)).contiguous()
              for _ in range(a.iters)]
    arms = ["f32", "f32_b"] + (["prev"] if prev else [])
    for k in KINDS:
        arms += [f"base_{k}", f"flag_{k}"]
    if a.only:
        assert a.only in arms and a.eager > 0
        arms = [a.only]

    with torch.no_grad(), torch.cuda.stream(stream):
        blocks = {"f32": dexiraft_amd.AlternateCorrBlock(f1, f2, num_levels=L, radius=r)}
        for k, (dt, mf) in KINDS.items():
            blocks[k] = dexiraft_amd.AlternateCorrBlock(f1, f2, num_levels=L, radius=r, out_dtype=dt,
                                                        memory_format=mf)
        ab = blocks["f32"]
        first = ab.coarse_first_level

        def prev_lookup(c):
            """AlternateCorrBlock._lookup's default calls, through the previous library."""
            out = torch.empty((B, L * 81, H, W), dtype=torch.float32, device=dev)
            s = stream.cuda_stream
            nl = L if first is None else first
            nb = prev.dxr_alt_workspace_bytes(B, H, W, nl)
            ws = torch.empty(max(nb, 0), dtype=torch.uint8, device=dev)
            if first is None:
                st = prev.dxr_alt_corr_lookup_ws(ab._f1_nhwc.data_ptr(), ab._f2_ptrs, c.data_ptr(),
                                                 out.data_ptr(), B, H, W, D, L, r, _sqrt_dim(D),
                                                 nat.ptr(ws), max(nb, 0), s)
                assert st == 0, st
                return out
            if first > 0:
                st = prev.dxr_alt_corr_lookup_levels_ws(ab._f1_nhwc.data_ptr(), ab._f2_ptrs,
                                                        c.data_ptr(), out.data_ptr(), B, H, W, D, L,
                                                        first, r, _sqrt_dim(D), nat.ptr(ws),
                                                        max(nb, 0), s)
                assert st == 0, st
            st = prev.dxr_alt_volume_lookup(ab._volumes.data_ptr(), c.data_ptr(), out.data_ptr(), B,
                                            H, W, L, first, r, _sqrt_dim(D), s)
            assert st == 0, st
            return out

        def lookup(arm, c):
            if arm == "prev":
                return prev_lookup(c)
            if arm.startswith("flag_"):
                return blocks[arm[5:]](c)
            o = ab(c)
            if arm.startswith("base_"):
                dt, mf = KINDS[arm[5:]]
                if dt is not None:
                    o = o.to(dt)
                if mf is not None:
                    o = o.contiguous(memory_format=CL)
            return o

        def step(arm):
            return [lookup(arm, c) for c in coords]   # every output alive: no reuse inside the graph

        if a.eager:
            for _ in range(a.eager):
                keep = step(arms[0])
                torch.cuda.synchronize()
                del keep
            print(json.dumps({"arm": arms[0], "eager_steps": a.eager, "lookups_per_step": a.iters,
                              "workload": a.workload, "coarse_first_level": first}))
            return

        def same(x, y):
            bits = torch.int32 if x.dtype == torch.float32 else torch.int16
            return (x.dtype == y.dtype and x.stride() == y.stride() and
                    torch.equal(x.permute(0, 2, 3, 1).contiguous().view(bits),
                                y.permute(0, 2, 3, 1).contiguous().view(bits)))

        ref = step("f32")
        torch.cuda.synchronize()
        if prev:
            assert all(same(x, y) for x, y in zip(step("prev"), ref)), "prev differs from f32"
        out_bytes = {"f32": ref[0].numel() * 4}
        del ref
        for k in KINDS:
            want, got = step(f"base_{k}"), step(f"flag_{k}")
            torch.cuda.synchronize()
            assert all(same(x, y) for x, y in zip(got, want)), k
            out_bytes[k] = got[0].numel() * got[0].element_size()
            del want, got
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
                res[v].append(e0.elapsed_time(e1) * 1e3 / a.reps / a.iters)
    med = {v: float(np.median(x)) for v, x in res.items()}
    # the noise floor: the largest difference of the two identical arms within one
    # round (a difference of two medians can be near zero by chance)
    spread = max(abs(x - y) for x, y in zip(res["f32"], res["f32_b"]))
    record = {
        "what": "us per lookup (a step graph of --iters lookups of one AlternateCorrBlock, "
                "divided by --iters), scripts/ab_alt_out.py",
        "workload": a.workload, "shape": [B, D, H, W], "radius": r, "num_levels": L,
        "coarse_first_level": first, "out_bytes_per_lookup": out_bytes,
        "iters": a.iters, "reps": a.reps, "rounds": a.rounds,
        "box": bench.box_identity(dev), "calibration": calib,
        "flagged_equals_converted_bitwise": True,
        "us_per_lookup_min_med_max": {v: [round(min(x), 2), round(med[v], 2), round(max(x), 2)]
                                      for v, x in res.items()},
        "aa_spread_us": round(spread, 3),
        "aa_spread_what": "max over rounds of |f32 - f32_b| within a round",
        "aa_median_difference_us": round(abs(med["f32_b"] - med["f32"]), 3),
        "aa_spread_rel": round(spread / med["f32"], 4),
        # 1. against the parent's way of getting the same tensor
        "flag_over_base_median": {k: round(med[f"flag_{k}"] / med[f"base_{k}"], 4) for k in KINDS},
        # 2. against the plain float32 NCHW lookup
        "flag_over_f32_median": {k: round(med[f"flag_{k}"] / med["f32"], 4) for k in KINDS},
    }
    if prev:   # 3. the default path against the parent commit's library
        record["prev_lib"] = str(a.prev_lib)
        record["f32_minus_prev_us"] = round(med["f32"] - med["prev"], 3)
        record["f32_b_minus_prev_us"] = round(med["f32_b"] - med["prev"], 3)
        record["default_within_aa_spread_of_prev"] = bool(
            max(abs(med["f32"] - med["prev"]), abs(med["f32_b"] - med["prev"])) <= spread)
    print(json.dumps(record), flush=True)
    if a.out:
        out = Path(a.out)
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(record, indent=1) + "\n")


if __name__ == "__main__":
    main()
