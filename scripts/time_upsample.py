#!/usr/bin/env python3
"""Time ``dexiraft_amd.upsample_flow`` against the reference's op sequence in torch
(profiles only).

Two arms on the same GPU in one process, interleaved round by round after a
clock warm-up:

  hip    dexiraft_amd.upsample_flow (csrc/flow_upsample.hip): one launch forward,
         two backward
  torch  tests/e2e_flow.upsample_flow, the restatement of core/raft.py:87-98:
         view -> softmax -> unfold -> multiply -> sum -> permute -> reshape, and
         what autograd records for it

Each arm runs twice per round (``hip``, ``torch``, ``hip_again``, ``torch_again``);
the difference between the two medians of one arm is its A/A spread, the noise
floor a difference between the arms has to clear.  Per case (shape x mask dtype)
two works are timed, the forward alone (under no_grad) and the forward plus the
backward of both inputs, each in two ways:

  graph_us  a captured graph of ``--graph-calls`` calls, replayed; device events,
            per call: the GPU time with the launches' host cost taken out
  eager_us  host clock around ``--calls`` eager calls and one device synchronise,
            per call: what a Python loop pays

Reported per arm: the median over rounds, the min-max of the rounds, every round.
``peak_extra_bytes``: the rise of torch's peak allocated memory over 12 forward
calls under autograd whose outputs are kept (a 12-iteration training step's
upsampling), per arm.  ``byte_floor_us``: the mask read once plus the output
written once (forward), or those plus grad_out and grad_mask (forward + backward),
at 6.3 TB/s.

Usage: python scripts/time_upsample.py
       (writes profiles/r18/upsample/<shape>_<dtype>.json unless --out-dir is given)
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
sys.path.insert(0, str(REPO / "tests"))

SHAPES = {"sintel_b1": (1, 55, 128), "chairs_b6": (6, 46, 62)}
DTYPES = {"float32": torch.float32, "float16": torch.float16}
ARMS = ("hip", "torch", "hip_again", "torch_again")
HBM_BYTES_PER_US = 6.3e6   # achievable HBM bandwidth, 6.3 TB/s


def summary(rounds: list[float]) -> dict:
    return {"median": statistics.median(rounds), "min": min(rounds), "max": max(rounds),
            "rounds": rounds}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--dtypes", nargs="+", default=list(DTYPES), choices=list(DTYPES))
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--calls", type=int, default=30, help="eager calls per arm and round")
    ap.add_argument("--graph-calls", type=int, default=12)
    ap.add_argument("--replays", type=int, default=10, help="graph replays per arm and round")
    ap.add_argument("--clock-warmup-s", type=float, default=0.5)
    ap.add_argument("--out-dir", default=str(REPO / "profiles" / "r18" / "upsample"))
    a = ap.parse_args()
    import dexiraft_amd
    import e2e_flow
    dexiraft_amd.load_native()
    if not torch.cuda.is_available():
        raise SystemExit("time_upsample.py needs a HIP device")
    dev = torch.device("cuda", 0)
    out_dir = Path(a.out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    fns = {"hip": dexiraft_amd.upsample_flow, "torch": e2e_flow.upsample_flow}
    for shape in a.shapes:
        N, H, W = SHAPES[shape]
        for dname in a.dtypes:
            dtype = DTYPES[dname]
            gen = torch.Generator(device=dev)
            gen.manual_seed(18)
            mask = torch.randn((N, 576, H, W), generator=gen, device=dev).to(dtype).requires_grad_()
            flow = (5 * torch.randn((N, 2, H, W), generator=gen, device=dev)).requires_grad_()
            gout = torch.randn((N, 2, 8 * H, 8 * W), generator=gen, device=dev)
            esz = mask.element_size()
            # forward: mask and flow read, out written; backward: mask, flow and grad_out read,
            # grad_mask written, the 18 T planes written and read, grad_flow written
            fwd_bytes = mask.numel() * esz + flow.numel() * 4 + gout.numel() * 4
            bwd_bytes = 2 * mask.numel() * esz + gout.numel() * 4 + (2 + 18 + 18 + 2) * N * H * W * 4
            rec = {"shape": shape, "N": N, "H": H, "W": W, "mask_dtype": dname,
                   "device": torch.cuda.get_device_name(dev), "rounds": a.rounds,
                   "calls_per_round": a.calls, "graph_calls": a.graph_calls,
                   "replays_per_round": a.replays,
                   "byte_floor_us": {"forward": fwd_bytes / HBM_BYTES_PER_US,
                                     "forward_backward": (fwd_bytes + bwd_bytes) / HBM_BYTES_PER_US}}

            def forward(fn):
                with torch.no_grad():
                    return fn(flow, mask)

            def forward_backward(fn):
                return torch.autograd.grad(fn(flow, mask), (flow, mask), gout)

            # agreement of the arms on the timed inputs
            o_h, o_t = forward(fns["hip"]), forward(fns["torch"])
            g_h, g_t = forward_backward(fns["hip"]), forward_backward(fns["torch"])
            rec["max_abs_diff"] = {"out": float((o_h - o_t).abs().max()),
                                   "grad_flow": float((g_h[0] - g_t[0]).abs().max()),
                                   "grad_mask": float((g_h[1].float() - g_t[1].float()).abs().max())}
            # memory: 12 forward calls under autograd, outputs kept
            rec["peak_extra_bytes"] = {}
            for arm, fn in fns.items():
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats(dev)
                base = torch.cuda.memory_allocated(dev)
                kept = [fn(flow, mask) for _ in range(12)]
                torch.cuda.synchronize()
                rec["peak_extra_bytes"][arm] = torch.cuda.max_memory_allocated(dev) - base
                del kept
            stream = torch.cuda.Stream(device=dev)
            stream.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(stream):
                for wname, work in (("forward", forward), ("forward_backward", forward_backward)):
                    graphs = {}
                    for arm, fn in fns.items():
                        work(fn)
                        graph = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(graph, stream=stream):
                            keep = [work(fn) for _ in range(a.graph_calls)]
                        graphs[arm] = (graph, keep)
                    t_end = time.perf_counter() + a.clock_warmup_s
                    while time.perf_counter() < t_end:
                        for graph, _ in graphs.values():
                            graph.replay()
                        stream.synchronize()
                    g_us = {arm: [] for arm in ARMS}
                    e_us = {arm: [] for arm in ARMS}
                    for _ in range(a.rounds):
                        for arm in ARMS:
                            graph, fn = graphs[arm.split("_")[0]][0], fns[arm.split("_")[0]]
                            e0 = torch.cuda.Event(enable_timing=True)
                            e1 = torch.cuda.Event(enable_timing=True)
                            e0.record(stream)
                            for _ in range(a.replays):
                                graph.replay()
                            e1.record(stream)
                            stream.synchronize()
                            g_us[arm].append(e0.elapsed_time(e1) * 1e3 / (a.replays * a.graph_calls))
                            t0 = time.perf_counter()
                            for _ in range(a.calls):
                                work(fn)
                            stream.synchronize()
                            e_us[arm].append((time.perf_counter() - t0) * 1e6 / a.calls)
                    res = {"graph_us": {arm: summary(v) for arm, v in g_us.items()},
                           "eager_us": {arm: summary(v) for arm, v in e_us.items()}}
                    for how in ("graph_us", "eager_us"):
                        r = res[how]
                        r["aa_spread_hip"] = abs(r["hip"]["median"] - r["hip_again"]["median"])
                        r["aa_spread_torch"] = abs(r["torch"]["median"] - r["torch_again"]["median"])
                        r["speedup"] = r["torch"]["median"] / r["hip"]["median"]
                    rec[wname] = res
                    del graphs
            torch.cuda.synchronize()
            (out_dir / f"{shape}_{dname}.json").write_text(json.dumps(rec, indent=1) + "\n")
            brief = {"shape": shape, "mask_dtype": dname, "byte_floor_us": rec["byte_floor_us"],
                     "peak_extra_bytes": rec["peak_extra_bytes"], "max_abs_diff": rec["max_abs_diff"]}
            for wname in ("forward", "forward_backward"):
                for how in ("graph_us", "eager_us"):
                    r = rec[wname][how]
                    brief[f"{wname}.{how}"] = {
                        "hip": [round(r["hip"][s], 2) for s in ("median", "min", "max")],
                        "torch": [round(r["torch"][s], 2) for s in ("median", "min", "max")],
                        "aa_hip": round(r["aa_spread_hip"], 2), "aa_torch": round(r["aa_spread_torch"], 2),
                        "speedup": round(r["speedup"], 2)}
            print(json.dumps(brief))


if __name__ == "__main__":
    main()
