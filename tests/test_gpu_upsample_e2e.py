"""GPU: the refinement loop of tests/e2e_flow.py around ``CorrBlock`` with its
convex upsampling replaced by ``dexiraft_amd.upsample_flow``, against the
reference loop's recorded flows (tests/golden/e2e_chairs.npz) under the criteria
of tests/test_e2e_flow.py: upsampled flow (``flow_up_sub4``) EPE < 8e-3 px,
per-iteration EPE < 1e-3 px."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import e2e_flow as ef
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

EPE_F32 = 1e-3      # px, the fp32 criterion of tests/test_e2e_flow.py


def test_e2e_corrblock_with_the_fused_upsampling(monkeypatch):
    import dexiraft_amd
    calls = []

    def upsample(flow, mask):
        calls.append(tuple(mask.shape))
        return dexiraft_amd.upsample_flow(flow, mask)

    monkeypatch.setattr(ef, "upsample_flow", upsample)
    x = ef.e2e_inputs()
    W = ef.torch_weights(ef.update_weights(), "cuda")
    t = {k: torch.from_numpy(v).to("cuda") for k, v in x.items()}
    with torch.no_grad():
        corr_fn = dexiraft_amd.CorrBlock(t["fmap1"], t["fmap2"])
        corr_en = dexiraft_amd.CorrBlock(t["fem1"], t["fem2"])
        flows, up, _ = ef.refine(corr_fn, corr_en, W, t)
    assert calls == [(1, 576, ef.E2E["H"], ef.E2E["W"])] * ef.E2E["iters"]
    with np.load(GOLDEN / "e2e_chairs.npz") as z:
        g = {k: z[k] for k in z.files}
    per_iter = [ef.epe(fl, g["flows"][i]) for i, fl in enumerate(flows)]
    up_epe = ef.epe(up[:, :, ::4, ::4], g["flow_up_sub4"])
    print(f"upsampled EPE {up_epe:.3e} px, max per-iteration EPE {max(per_iter):.3e} px")
    assert up.shape == (1, 2, 8 * ef.E2E["H"], 8 * ef.E2E["W"])
    assert np.isfinite(up_epe) and up_epe < 8 * EPE_F32
    assert max(per_iter) < EPE_F32, per_iter
