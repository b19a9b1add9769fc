#!/usr/bin/env python3
"""Times the backward of TrainableAlternateCorrBlock (profiles only).

One process, HIP events, interleaved rounds after a clock warm-up.  A step is
the full backward of ``--iters`` lookups (12) of one block through autograd
(``torch.autograd.grad`` of all lookup outputs with respect to both fmaps) at
D = 256, r = 4, 4 levels, on two flow models: the benchmark's i.i.d.
N(0, 4^2) displacements per pixel and a smooth flow (a low-frequency field of
the same amplitude, as real flow is).

Arms:
  mfma              the product path: ``dxr_alt_corr_backward`` with
                    ``DXR_ALT_BWD_ACCUMULATE`` (csrc/alt_corr_bwd.hip)
  base, base_b      the same autograd path forced onto the unflagged entry point
                    (the per-query atomic kernel plus torch adds), twice: the
                    A/A whose largest difference within a round is the noise
                    floor
Before anything is timed the two paths' gradients are compared.  At the Sintel
size the peak extra memory of a training step (forward of the lookups plus
their backward, above the fmaps) is recorded beside ``CorrBlock``'s.

Usage: python scripts/time_alt_backward.py --workload sintel --out profiles/.../x.json
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

SHAPES = {"sintel": (55, 128), "1080p": (136, 240)}


def flows(kind, B, H, W, iters, dev, g):
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32),
                            torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    grid = torch.stack((xs, ys))[None].expand(B, 2, H, W)
    out = []
    for _ in range(iters):
        if kind == "iid":
            d = 4.0 * torch.randn((B, 2, H, W), generator=g, device=dev)
        else:   # smooth: an 8 x-coarser normal field, bilinearly upsampled
            lo = 4.0 * torch.randn((B, 2, (H + 7) // 8 + 1, (W + 7) // 8 + 1), generator=g,
                                   device=dev)
            d = torch.nn.functional.interpolate(lo, size=(H, W), mode="bilinear",
                                                align_corners=True)
        out.append((grid + d).contiguous())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="sintel", choices=sorted(SHAPES))
    ap.add_argument("--iters", type=int, default=12, help="lookups per step")
    ap.add_argument("--reps", type=int, default=3, help="steps per timed round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="write the JSON record here too")
    a = ap.parse_args()
    import dexiraft_amd as dx
    dx.load_native()
    if not torch.cuda.is_available():
        raise SystemExit("time_alt_backward.py needs a HIP device")
    dev = torch.device("cuda", 0)
    B, (H, W), D, L, r = 1, SHAPES[a.workload], 256, 4, 4
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    f1 = torch.randn((B, D, H, W), generator=g, device=dev).requires_grad_(True)
    f2 = torch.randn((B, D, H, W), generator=g, device=dev).requires_grad_(True)
    gouts = [torch.randn((B, L * 81, H, W), generator=g, device=dev) for _ in range(a.iters)]
    rec = {"workload": a.workload, "shape": [B, D, H, W], "levels": L, "radius": r,
           "iters": a.iters, "reps": a.reps, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "flows": {}}

    def make(native):
        blk = dx.TrainableAlternateCorrBlock(f1, f2, L, r)
        blk._bwd_native = native      # False: every level through the unflagged entry point
        return blk

    def step(blk, outs):
        return torch.autograd.grad(outs, [f1, f2], gouts, retain_graph=True)

    for kind in ("iid", "smooth"):
        cs = flows(kind, B, H, W, a.iters, dev, g)
        arms = {"mfma": make(True), "base": make(False), "base_b": make(False)}
        outs = {k: [b(c) for c in cs] for k, b in arms.items()}
        # the two paths compute the same gradients (summation order apart)
        gm, gb = step(arms["mfma"], outs["mfma"]), step(arms["base"], outs["base"])
        agree = [float(((x - y).abs().max() / y.abs().max()).item()) for x, y in zip(gm, gb)]
        assert arms["mfma"]._bwd_native and max(agree) < 1e-4, agree
        for _ in range(3):                                    # clock and allocator warm-up
            for k in arms:
                step(arms[k], outs[k])
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        order = list(arms)
        for rd in range(a.rounds):
            for k in order[rd % 3:] + order[:rd % 3]:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    step(arms[k], outs[k])
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) / a.reps)
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        aa = max(abs(x - y) / min(x, y) for x, y in zip(times["base"], times["base_b"]))
        rec["flows"][kind] = {
            "ms_per_backward_step": times, "median_ms": med, "aa_spread": aa,
            "speedup_median": med["base"] / med["mfma"],
            "speedup_min_round": min(x / y for x, y in zip(times["base"], times["mfma"])),
            "max_rel_diff_vs_base": agree}
        print(f"{a.workload} {kind}: mfma {med['mfma']:.3f} ms, base {med['base']:.3f} / "
              f"{med['base_b']:.3f} ms per {a.iters}-lookup backward; A/A spread {aa:.2%}; "
              f"speedup {med['base'] / med['mfma']:.2f}x")
        del arms, outs, gm, gb

    if a.workload == "sintel":
        # peak extra memory of a training step (block, 12 lookups, backward) above the fmaps
        cs = flows("iid", B, H, W, a.iters, dev, g)
        peaks = {}
        for name, cls in (("TrainableAlternateCorrBlock", dx.TrainableAlternateCorrBlock),
                          ("CorrBlock", dx.CorrBlock)):
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            blk = cls(f1, f2, L, r)
            loss = sum((blk(c) * go).sum() for c, go in zip(cs, gouts))
            grads = torch.autograd.grad(loss, [f1, f2])
            torch.cuda.synchronize()
            peaks[name] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
            del blk, loss, grads
        rec["peak_extra_MiB_training_step"] = peaks
        print("peak extra MiB of a training step:", peaks)

    line = json.dumps(rec)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
