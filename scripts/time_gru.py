#!/usr/bin/env python3
"""Time ``dexiraft_amd.SepConvGRU`` against the reference's op sequence in torch
(profiles only).

Three arms on the same GPU in one process, interleaved round by round after a
clock warm-up:

  hip        dexiraft_amd.SepConvGRU (csrc/gru_sepconv.hip): five launches
  torch      the op sequence of core/update.py:45-60 restated here (two cats, six
             convolutions, the pointwise gates) in float32
  autocast   the same sequence under torch.autocast of the compute dtype, float32
             inputs and parameters, as --mixed_precision runs it

Each arm runs twice per round (``hip``, ``torch``, ``autocast``, ``hip_again``, ...);
the difference between the two medians of one arm is its A/A spread, the noise
floor a difference between the arms has to clear.  Every arm is timed inside a
captured graph of ``--graph-calls`` calls, replayed; device events, per call: the
GPU time with the launches' host cost taken out.

Reported per arm: the median over rounds, the min-max of the rounds, every round.
``peak_extra_bytes``: the rise of torch's peak allocated memory over one call
above the inputs, parameters and (for hip) packed weights, per arm.

Usage: python scripts/time_gru.py
       (writes profiles/r22/gru/<shape>_<dtype>.json unless --out-dir is given)
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

SHAPES = {"sintel_b1": (1, 55, 128), "sintel_b2": (2, 55, 128), "chairs_b6": (6, 46, 62)}
DTYPES = {"bfloat16": torch.bfloat16, "float16": torch.float16}
BASE = ("hip", "torch", "autocast")
ARMS = BASE + tuple(f"{a}_again" for a in BASE)
NAMES = ("convz1", "convr1", "convq1", "convz2", "convr2", "convq2")
CH, CX = 128, 256


def torch_gru(p, h, x):
    """core/update.py:45-60 on the parameter dict p."""
    import torch.nn.functional as F

    def conv(name, t):
        pad = (0, 2) if name.endswith("1") else (2, 0)
        return F.conv2d(t, p[f"{name}.weight"], p[f"{name}.bias"], padding=pad)

    for a in ("1", "2"):
        hx = torch.cat([h, x], dim=1)
        z = torch.sigmoid(conv("convz" + a, hx))
        r = torch.sigmoid(conv("convr" + a, hx))
        q = torch.tanh(conv("convq" + a, torch.cat([r * h, x], dim=1)))
        h = (1 - z) * h + z * q
    return h


def summary(rounds: list[float]) -> dict:
    return {"median": statistics.median(rounds), "min": min(rounds), "max": max(rounds),
            "rounds": rounds}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--dtypes", nargs="+", default=list(DTYPES), choices=list(DTYPES))
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--graph-calls", type=int, default=12)
    ap.add_argument("--replays", type=int, default=5, help="graph replays per arm and round")
    ap.add_argument("--clock-warmup-s", type=float, default=0.5)
    ap.add_argument("--out-dir", default=str(REPO / "profiles" / "r22" / "gru"))
    a = ap.parse_args()
    import dexiraft_amd
    if not torch.cuda.is_available():
        raise SystemExit("time_gru.py needs a HIP device")
    dev = torch.device("cuda", 0)
    out_dir = Path(a.out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    gen = torch.Generator(device=dev)
    gen.manual_seed(22)
    K = 5 * (CH + CX)
    params = {}
    for i, n in enumerate(NAMES):
        shape = (CH, CH + CX, 1, 5) if i < 3 else (CH, CH + CX, 5, 1)
        params[f"{n}.weight"] = torch.randn(shape, generator=gen, device=dev) / K ** 0.5
        params[f"{n}.bias"] = 0.5 * torch.randn(CH, generator=gen, device=dev)
    for shape in a.shapes:
        N, H, W = SHAPES[shape]
        h = torch.tanh(torch.randn((N, CH, H, W), generator=gen, device=dev))
        x = torch.randn((N, CX, H, W), generator=gen, device=dev)
        for dname in a.dtypes:
            c = DTYPES[dname]
            hip = dexiraft_amd.SepConvGRU(params, compute_dtype=c)

            def run_autocast(h, x, c=c):
                with torch.autocast("cuda", dtype=c):
                    return torch_gru(params, h, x)

            fns = {"hip": hip, "torch": lambda h, x: torch_gru(params, h, x),
                   "autocast": run_autocast}
            rec = {"shape": shape, "N": N, "H": H, "W": W, "Ch": CH, "Cx": CX,
                   "compute_dtype": dname, "device": torch.cuda.get_device_name(dev),
                   "rounds": a.rounds, "graph_calls": a.graph_calls,
                   "replays_per_round": a.replays, "gflop_per_call": 2 * N * H * W * 6 * CH * K / 1e9}
            with torch.no_grad():
                outs = {arm: fn(h, x).float() for arm, fn in fns.items()}   # warm-up, packing
                rec["max_abs_diff_vs_torch"] = {arm: float((outs[arm] - outs["torch"]).abs().max())
                                                for arm in ("hip", "autocast")}
                rec["peak_extra_bytes"] = {}
                for arm, fn in fns.items():
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats(dev)
                    base = torch.cuda.memory_allocated(dev)
                    fn(h, x)
                    torch.cuda.synchronize()
                    rec["peak_extra_bytes"][arm] = torch.cuda.max_memory_allocated(dev) - base
                stream = torch.cuda.Stream(device=dev)
                stream.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(stream):
                    graphs = {}
                    for arm, fn in fns.items():
                        fn(h, x)
                        graph = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(graph, stream=stream):
                            keep = [fn(h, x) for _ in range(a.graph_calls)]
                        graphs[arm] = (graph, keep)
                    t_end = time.perf_counter() + a.clock_warmup_s
                    while time.perf_counter() < t_end:
                        for graph, _ in graphs.values():
                            graph.replay()
                        stream.synchronize()
                    g_us = {arm: [] for arm in ARMS}
                    for _ in range(a.rounds):
                        for arm in ARMS:
                            graph = graphs[arm.split("_")[0]][0]
                            e0 = torch.cuda.Event(enable_timing=True)
                            e1 = torch.cuda.Event(enable_timing=True)
                            e0.record(stream)
                            for _ in range(a.replays):
                                graph.replay()
                            e1.record(stream)
                            stream.synchronize()
                            g_us[arm].append(e0.elapsed_time(e1) * 1e3 / (a.replays * a.graph_calls))
                    del graphs
                torch.cuda.current_stream(dev).wait_stream(stream)
            res = {arm: summary(v) for arm, v in g_us.items()}
            for arm in BASE:
                res[f"aa_spread_{arm}"] = abs(res[arm]["median"] - res[f"{arm}_again"]["median"])
            res["speedup_vs_torch"] = res["torch"]["median"] / res["hip"]["median"]
            res["speedup_vs_autocast"] = res["autocast"]["median"] / res["hip"]["median"]
            res["hip_tflops"] = rec["gflop_per_call"] / res["hip"]["median"] * 1e3
            rec["graph_us"] = res
            torch.cuda.synchronize()
            (out_dir / f"{shape}_{dname}.json").write_text(json.dumps(rec, indent=1) + "\n")
            brief = {"shape": shape, "compute_dtype": dname,
                     "peak_extra_bytes": rec["peak_extra_bytes"],
                     "max_abs_diff_vs_torch": rec["max_abs_diff_vs_torch"]}
            for arm in BASE:
                brief[arm] = [round(res[arm][s], 2) for s in ("median", "min", "max")]
                brief[f"aa_{arm}"] = round(res[f"aa_spread_{arm}"], 2)
            brief["speedup_vs_torch"] = round(res["speedup_vs_torch"], 2)
            brief["speedup_vs_autocast"] = round(res["speedup_vs_autocast"], 2)
            brief["hip_tflops"] = round(res["hip_tflops"], 1)
            print(json.dumps(brief), flush=True)


if __name__ == "__main__":
    main()
