#!/usr/bin/env python3
"""Time one ``forward_interpolate`` call against the reference's (profiles only).

What a warm-start loop pays per frame pair for pushing ``flow_low`` forward
(evaluate.py:44): here ``dexiraft_amd.forward_interpolate(flow_low[0])[None]``,
which stays on the GPU; in the reference ``forward_interpolate(flow_low[0])[None]
.cuda()`` — a device-to-host copy, two scipy ``griddata(method='nearest')`` calls
and the copy back (core/utils/utils.py:26-54).  One process, B = 1, after a clock
warm-up, the arms interleaved round by round:

  gpu_call_us        host clock around one call + a device synchronise (what an
                     eager loop that needs the result pays), median of the round
  gpu_graph_us       a captured graph of ``--graph-calls`` calls, replayed;
                     device events, per call
  reference_call_us  host clock around the reference's call with both copies and
                     a device synchronise, median of the round

Reported per arm: the median over rounds and the min-max spread of the rounds.
The reference's function is imported from a reference checkout (``--reference
DIR``, its ``core/`` on sys.path; scipy needed); without it only the GPU arms run.
Before timing, the output is compared with the reference's cell by cell.

Usage: python scripts/time_forward_interp.py --reference DIR
       (writes profiles/r17/flow_interp/<shape>.json unless --out-dir is given)
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

SHAPES = {"sintel": (55, 128), "1080p": (135, 240)}


def summary(rounds: list[float]) -> dict:
    return {"median": statistics.median(rounds), "min": min(rounds), "max": max(rounds),
            "rounds": rounds}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None, help="root of a reference checkout")
    ap.add_argument("--shapes", nargs="+", default=sorted(SHAPES), choices=sorted(SHAPES))
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=40, help="GPU calls per round (eager arm)")
    ap.add_argument("--ref-calls", type=int, default=3, help="reference calls per round")
    ap.add_argument("--graph-calls", type=int, default=10)
    ap.add_argument("--replays", type=int, default=20, help="graph replays per round")
    ap.add_argument("--sigma", type=float, default=3.0, help="flow sigma, px")
    ap.add_argument("--clock-warmup-s", type=float, default=0.5)
    ap.add_argument("--out-dir", default=str(REPO / "profiles" / "r17" / "flow_interp"))
    a = ap.parse_args()
    import dexiraft_amd
    dexiraft_amd.load_native()
    if not torch.cuda.is_available():
        raise SystemExit("time_forward_interp.py needs a HIP device")
    ref_fi = None
    if a.reference:
        sys.path.insert(0, str(Path(a.reference) / "core"))
        from utils.utils import forward_interpolate as ref_fi   # the reference's own function
    dev = torch.device("cuda", 0)
    out_dir = Path(a.out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    fi = dexiraft_amd.forward_interpolate
    for name in a.shapes:
        H, W = SHAPES[name]
        g = torch.Generator(device=dev)
        g.manual_seed(17)
        flow_low = (a.sigma * torch.randn((1, 2, H, W), generator=g, device=dev)).contiguous()
        rec = {"shape": name, "H": H, "W": W, "B": 1, "sigma_px": a.sigma,
               "device": torch.cuda.get_device_name(dev), "rounds": a.rounds,
               "calls_per_round": a.calls, "ref_calls_per_round": a.ref_calls,
               "graph_calls": a.graph_calls, "replays_per_round": a.replays}
        ours = fi(flow_low[0])[None]
        if ref_fi is not None:
            theirs = ref_fi(flow_low[0])[None].to(dev)
            rec["cells_differing_from_reference"] = int((ours != theirs).sum())
        stream = torch.cuda.Stream(device=dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.no_grad(), torch.cuda.stream(stream):
            fi(flow_low[0])
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                outs = [fi(flow_low[0]) for _ in range(a.graph_calls)]
            graph.replay()
            stream.synchronize()
            assert all(torch.equal(o, ours[0]) for o in outs)
            t_end = time.perf_counter() + a.clock_warmup_s
            while time.perf_counter() < t_end:
                graph.replay()
                stream.synchronize()
            arms = {"gpu_call_us": [], "gpu_graph_us": [], "reference_call_us": []}
            for _ in range(a.rounds):
                ts = []
                for _ in range(a.calls):
                    t0 = time.perf_counter()
                    fi(flow_low[0])[None]
                    stream.synchronize()
                    ts.append((time.perf_counter() - t0) * 1e6)
                arms["gpu_call_us"].append(statistics.median(ts))
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.replays):
                    graph.replay()
                e1.record(stream)
                stream.synchronize()
                arms["gpu_graph_us"].append(e0.elapsed_time(e1) * 1e3
                                            / (a.replays * a.graph_calls))
                if ref_fi is not None:
                    ts = []
                    for _ in range(a.ref_calls):
                        t0 = time.perf_counter()
                        ref_fi(flow_low[0])[None].to(dev)
                        stream.synchronize()
                        ts.append((time.perf_counter() - t0) * 1e6)
                    arms["reference_call_us"].append(statistics.median(ts))
        for arm, rounds in arms.items():
            if rounds:
                rec[arm] = summary(rounds)
        if ref_fi is not None:
            rec["speedup_call"] = rec["reference_call_us"]["median"] / rec["gpu_call_us"]["median"]
        (out_dir / f"{name}.json").write_text(json.dumps(rec, indent=1) + "\n")
        print(json.dumps({k: (v if not isinstance(v, dict) else
                              {s: round(v[s], 2) for s in ("median", "min", "max")})
                          for k, v in rec.items()}))


if __name__ == "__main__":
    main()
