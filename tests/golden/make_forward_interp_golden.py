"""Golden inputs and outputs of the REFERENCE forward_interpolate (core/utils/utils.py:26-54).

Run where the reference checkout and scipy exist:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_forward_interp_golden.py --reference DIR
Records, for 6x8, 13x17 and 24x40, a flow (continuous random, sigma 3 px, plus a
smooth ramp, so that some sources leave the frame) and what the reference's own
function returns for it, into tests/golden/forward_interp.npz (data only).

scipy's KD-tree leaves ties unspecified, and its distances are not computed by
the float64 rule of include/dexiraft_flow.h, so a grid point whose best and
second-best d2 (among sources with a different flow value) agree to a relative
1e-12 may legitimately differ.  The script runs the float64 rule (the oracle of
tests/test_gpu_flow_interp.py) on every input and asserts, here on the CPU, that
the share of such near-tied grid points is at most 1 % and that the reference
equals the rule at every other cell: the cap the GPU test applies is then met by
the reference alone.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
SHAPES = [(6, 8), (13, 17), (24, 40)]
SIGMA = 3.0
NEAR_TIE_CAP = 0.01


def make_flow(seed: int, h: int, w: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    f = rng.normal(0.0, SIGMA, size=(2, h, w))
    ys, xs = np.meshgrid(np.linspace(-1.0, 1.0, h), np.linspace(-1.0, 1.0, w), indexing="ij")
    f[0] += 0.35 * w * xs * np.abs(xs)      # pushes the left and right borders outwards
    f[1] += 0.25 * h * np.sin(2.0 * ys)
    return f.astype(np.float32)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout")
    a = ap.parse_args()
    sys.path.insert(0, str(Path(a.reference) / "core"))
    sys.path.insert(0, str(HERE.parent))
    import torch
    from utils.utils import forward_interpolate   # the reference's own function
    from test_gpu_flow_interp import oracle_forward_interpolate

    out = {}
    for k, (h, w) in enumerate(SHAPES):
        flow = make_flow(1700 + k, h, w)
        ref = forward_interpolate(torch.from_numpy(flow)).numpy()
        assert ref.shape == flow.shape and ref.dtype == np.float32
        ours, near = oracle_forward_interpolate(flow, want_near=True)
        share = float(near.mean())
        x1 = np.arange(w)[None, :] + flow[0].astype(np.float64)
        y1 = np.arange(h)[:, None] + flow[1].astype(np.float64)
        left = int(((x1 > 0) & (x1 < w) & (y1 > 0) & (y1 < h)).sum())
        print(f"{h}x{w}: {left} of {h * w} sources stay inside, near-tied share {share:.4f}")
        assert 0 < left < h * w
        assert share <= NEAR_TIE_CAP
        keep = ~near
        assert np.array_equal(ref[:, keep], ours[:, keep])
        out[f"flow_{h}x{w}"] = flow
        out[f"ref_{h}x{w}"] = ref
    path = HERE / "forward_interp.npz"
    np.savez(path, **out)
    size = path.stat().st_size
    print(f"{path.name}: {size} bytes")
    assert size < 64 * 1024


if __name__ == "__main__":
    main()
