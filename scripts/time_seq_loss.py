#!/usr/bin/env python3
"""Time ``dexiraft_amd.sequence_loss`` against the torch op sequence of the same
definition (profiles only).

Two arms on the same GPU in one process, interleaved round by round after a
clock warm-up:

  hip    dexiraft_amd.sequence_loss(..., sync_metrics=False) (csrc/flow_loss.hip):
         two launches forward, one backward
  torch  tests/loss_oracle.torch_sequence, the definition of train.py:48-73 as
         torch ops (sub, abs, mask multiply, mean, scale, add per prediction; the
         statistics as masked sums, without the reference's four .item() calls, so
         that it can be captured), and what autograd records for it

Each arm runs twice per round (``hip``, ``torch``, ``hip_again``, ``torch_again``);
the difference between the two medians of one arm is its A/A spread, the noise
floor a difference between the arms has to clear.  Per shape two works are timed,
the forward alone (under no_grad) and the forward plus the backward into all P
predictions, each in two ways:

  graph_us  a captured graph of ``--graph-calls`` calls, replayed; device events,
            per call: the GPU time with the launches' host cost taken out
  eager_us  host clock around ``--calls`` eager calls and one device synchronise,
            per call: what a Python loop pays

Reported per arm: the median over rounds, the min-max of the rounds, every round.
``peak_extra_bytes``: the rise of torch's peak allocated memory over one forward +
backward above the inputs, per arm (the P gradients are 8*B*H*W*P bytes of it).
``byte_floor_us``: every prediction, flow_gt and valid read once (forward), and
those again plus the gradients written (forward + backward), at 6.3 TB/s.

Usage: python scripts/time_seq_loss.py
       (writes profiles/r19/seq_loss/<shape>.json unless --out-dir is given)
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

SHAPES = {"chairs_b6": (6, 368, 496), "sintel_b6": (6, 368, 768)}
ARMS = ("hip", "torch", "hip_again", "torch_again")
HBM_BYTES_PER_US = 6.3e6   # achievable HBM bandwidth, 6.3 TB/s
GAMMA, MAX_FLOW = 0.8, 400.0


def summary(rounds: list[float]) -> dict:
    return {"median": statistics.median(rounds), "min": min(rounds), "max": max(rounds),
            "rounds": rounds}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--preds", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--calls", type=int, default=20, help="eager calls per arm and round")
    ap.add_argument("--graph-calls", type=int, default=4)
    ap.add_argument("--replays", type=int, default=10, help="graph replays per arm and round")
    ap.add_argument("--clock-warmup-s", type=float, default=0.5)
    ap.add_argument("--out-dir", default=str(REPO / "profiles" / "r19" / "seq_loss"))
    a = ap.parse_args()
    import dexiraft_amd
    import loss_oracle
    dexiraft_amd.load_native()
    if not torch.cuda.is_available():
        raise SystemExit("time_seq_loss.py needs a HIP device")
    dev = torch.device("cuda", 0)
    out_dir = Path(a.out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)

    def hip(preds, gt, valid):
        loss, m = dexiraft_amd.sequence_loss(preds, gt, valid, GAMMA, MAX_FLOW, sync_metrics=False)
        return loss, m["stats"]

    def torch_arm(preds, gt, valid):
        return loss_oracle.torch_sequence(preds, gt, valid, GAMMA, MAX_FLOW)

    fns = {"hip": hip, "torch": torch_arm}
    for shape in a.shapes:
        B, H, W = SHAPES[shape]
        P = a.preds
        gen = torch.Generator(device=dev)
        gen.manual_seed(19)
        gt = 30 * torch.randn((B, 2, H, W), generator=gen, device=dev)
        valid = (torch.rand((B, H, W), generator=gen, device=dev) < 0.8).float()
        preds = [(gt + 2 * torch.randn((B, 2, H, W), generator=gen, device=dev)).requires_grad_()
                 for _ in range(P)]
        plane = B * H * W * 4
        fwd_bytes = (2 * P + 3) * plane
        bwd_bytes = (2 * P + 3) * plane + 2 * P * plane
        rec = {"shape": shape, "B": B, "H": H, "W": W, "P": P,
               "device": torch.cuda.get_device_name(dev), "rounds": a.rounds,
               "calls_per_round": a.calls, "graph_calls": a.graph_calls,
               "replays_per_round": a.replays,
               "byte_floor_us": {"forward": fwd_bytes / HBM_BYTES_PER_US,
                                 "forward_backward": (fwd_bytes + bwd_bytes) / HBM_BYTES_PER_US}}

        def forward(fn):
            with torch.no_grad():
                return fn(preds, gt, valid)

        def forward_backward(fn):
            loss, stats = fn(preds, gt, valid)
            return (loss.detach(), stats, *torch.autograd.grad(loss, preds))

        # agreement of the arms on the timed inputs
        o_h, o_t = forward_backward(fns["hip"]), forward_backward(fns["torch"])
        rec["agreement"] = {
            "loss_hip": float(o_h[0]), "loss_torch": float(o_t[0]),
            "stats_hip": o_h[1].tolist(), "stats_torch": o_t[1].tolist(),
            "max_abs_grad_diff": max(float((x - y).abs().max()) for x, y in zip(o_h[2:], o_t[2:])),
            "max_abs_grad": max(float(y.abs().max()) for y in o_t[2:])}
        del o_h, o_t
        # memory: one forward + backward above the inputs
        rec["peak_extra_bytes"] = {}
        for arm, fn in fns.items():
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            kept = forward_backward(fn)
            torch.cuda.synchronize()
            rec["peak_extra_bytes"][arm] = torch.cuda.max_memory_allocated(dev) - base
            del kept
        rec["gradient_bytes"] = 2 * P * plane
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
        (out_dir / f"{shape}.json").write_text(json.dumps(rec, indent=1) + "\n")
        brief = {"shape": shape, "P": P, "byte_floor_us": rec["byte_floor_us"],
                 "peak_extra_bytes": rec["peak_extra_bytes"], "agreement": rec["agreement"]}
        for wname in ("forward", "forward_backward"):
            for how in ("graph_us", "eager_us"):
                r = rec[wname][how]
                brief[f"{wname}.{how}"] = {
                    "hip": [round(r["hip"][s], 2) for s in ("median", "min", "max")],
                    "torch": [round(r["torch"][s], 2) for s in ("median", "min", "max")],
                    "aa_hip": round(r["aa_spread_hip"], 2), "aa_torch": round(r["aa_spread_torch"], 2),
                    "speedup": round(r["speedup"], 2)}
        print(json.dumps(brief), flush=True)
        del preds, gt, valid


if __name__ == "__main__":
    main()
