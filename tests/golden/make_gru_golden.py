"""Golden vectors for the fused SepConvGRU forward, from the REFERENCE
core/update.py on CPU in float32.

Run in the build container (where /root/reference exists):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_gru_golden.py
For each case: h, x and the six convolutions' parameters from
tests/gru_oracle.case (seeded), the reference's own ``SepConvGRU`` with those
parameters, one forward.  Inputs are regenerated from the seed at test time; the
recorded output is the fixture.
"""
from __future__ import annotations

import sys
import warnings
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
REFERENCE = Path("/root/reference/core")

import gru_oracle as go  # noqa: E402

# name: (seed, N, H, W, Ch, Cx)
CASES = {
    "gru_c16_b2": (7100, 2, 5, 7, 16, 32),
    "gru_c32": (7200, 1, 4, 9, 32, 64),
}


def main() -> None:
    warnings.filterwarnings("ignore")
    sys.path.insert(0, str(REFERENCE))
    import torch
    import update  # the reference's own module
    torch.set_num_threads(8)
    for name, (seed, N, H, W, Ch, Cx) in CASES.items():
        h, x, weights = go.case(seed, N, H, W, Ch, Cx)
        gru = update.SepConvGRU(hidden_dim=Ch, input_dim=Cx)
        gru.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
        with torch.no_grad():
            out = gru(torch.from_numpy(h), torch.from_numpy(x))   # core/update.py:45-60
        np.savez_compressed(
            HERE / f"{name}.npz", case=np.array([seed, N, H, W, Ch, Cx]),
            input_checksum=np.array([h.astype(np.float64).sum(), x.astype(np.float64).sum()]),
            out=out.numpy().astype(np.float32))
        print(name, tuple(out.shape), float(out.abs().max()))


if __name__ == "__main__":
    main()
