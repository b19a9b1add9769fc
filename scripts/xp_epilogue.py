#!/usr/bin/env python3
"""Build epilogue: what the level-0 LDS staging stores cost (experiments target).

``dxr_xp_build_epi`` of csrc/experiments/xp_build.hip launches the product's DMA
build (split pass or none, grid, tail, store policy as the package launches it)
with or without its level-0 staging stores (``nostage``: the global stores then
write whatever the staging region holds — timing only).  Several experiments
libraries can be timed side by side (``--lib LABEL=PATH``, e.g. one built from
an earlier commit's staging), each as LABEL, LABEL_nostage and LABEL_null (the
same graph as LABEL captured a second time: the null A/B of the session).  The
unablated builds of all libraries must give bit-identical pyramids.

Each variant is a HIP graph of --reps back-to-back builds; the graphs are
replayed in interleaved rounds after a clock warm-up (HIP events).
Usage: python scripts/xp_epilogue.py --lib new=PATH [--lib old=PATH]
           [--configs f32:1x55x128 f32:8x55x128 bf16:8x47x156]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", action="append", default=[], help="LABEL=PATH of an experiments library")
    ap.add_argument("--configs", nargs="+",
                    default=["f32:1x55x128", "f32:8x55x128", "bf16:8x47x156"],
                    help="DTYPE:BxHxW (f32: NCHW fmaps; bf16: channels-last fmaps)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    import dexiraft_amd
    from dexiraft_amd import _native as nat
    plib = dexiraft_amd.load_native()
    if not a.lib:
        a.lib = ["new=" + str(nat.LIB_PATH.with_name("libdexiraft_corr_exp.so"))]
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    libs = {}
    for spec in a.lib:
        label, path = spec.split("=", 1)
        lib = ctypes.CDLL(path)
        lib.dxr_xp_build_epi.restype = i32
        lib.dxr_xp_build_epi.argtypes = [vp, vp, i32, i64, i64, i64, i64, vp, vp, i32, vp]
        libs[label] = lib
    dev = torch.device("cuda", 0)
    D = 256
    stream = torch.cuda.Stream(device=dev)
    for cfg in a.configs:
        dtype, shp = cfg.split(":")
        B, H, W = (int(v) for v in shp.split("x"))
        g = torch.Generator(device=dev)
        g.manual_seed(7)
        f1 = torch.randn((B, D, H, W), generator=g, device=dev)
        f2 = torch.randn((B, D, H, W), generator=g, device=dev)
        dt = nat.DXR_F32
        if dtype == "bf16":
            f1 = f1.bfloat16().contiguous(memory_format=torch.channels_last)
            f2 = f2.bfloat16().contiguous(memory_format=torch.channels_last)
            dt = nat.DXR_BF16
        pyr = torch.empty(plib.dxr_pyramid_numel(B, H, W, 4), device=dev,
                          dtype=torch.float32 if dt == nat.DXR_F32 else torch.bfloat16)
        wsb = plib.dxr_build_workspace_bytes(dt, B, D, H, W) if dt == nat.DXR_F32 else 0
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)

        def build(v):
            label, _, kind = v.partition("_")
            st = libs[label].dxr_xp_build_epi(f1.data_ptr(), f2.data_ptr(), dt, B, D, H, W,
                                              pyr.data_ptr(), ws.data_ptr(),
                                              1 if kind == "nostage" else 0, stream.cuda_stream)
            assert st == 0, (v, st)

        variants = [f"{label}{k}" for label in libs for k in ("", "_nostage", "_null")]
        graphs, ref = {}, None
        with torch.cuda.stream(stream):
            for v in variants:
                build(v)
                torch.cuda.synchronize()
                if not v.endswith("_nostage"):
                    if ref is None:
                        ref = pyr.clone()
                    assert torch.equal(torch.nan_to_num(pyr.float(), nan=3.0),
                                       torch.nan_to_num(ref.float(), nan=3.0)), v
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr, stream=stream):
                    for _ in range(a.reps):
                        build(v)
                graphs[v] = gr
            for _ in range(10):
                for v in variants:
                    graphs[v].replay()
            torch.cuda.synchronize()
            res = {v: [] for v in variants}
            for _ in range(a.rounds):
                for v in variants:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    graphs[v].replay()
                    e1.record(stream)
                    torch.cuda.synchronize()
                    res[v].append(e0.elapsed_time(e1) * 1e3 / a.reps)
        print(json.dumps({"config": cfg, "D": D, "rounds": a.rounds, "reps": a.reps,
                          "unablated_pyramids_bit_identical": True,
                          "us_per_build_min_med": {v: [round(min(x), 1), round(float(np.median(x)), 1)]
                                                   for v, x in res.items()}}), flush=True)


if __name__ == "__main__":
    main()
