"""bench.py's command line: a plain run carries the headline figure only, ``--full``
adds the other measurements, ``--steps`` sets the number of timed steps, and
``--dump-outputs`` writes what the last timed step's lookups returned."""
from __future__ import annotations

import json
import sys

import numpy as np
import pytest
import torch

import bench

MAX_DUMP_BYTES = 64 << 20
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "lookup_roofline", "cpu_baseline")


def _sample(numel, n):
    return np.sort(np.random.default_rng(bench.DUMP_SAMPLE_SEED).choice(numel, n, replace=False))


def test_dump_outputs_whole_when_small(tmp_path):
    outs = [torch.arange(24, dtype=torch.float32).reshape(1, 2, 3, 4) + k for k in range(12)]
    bench.dump_outputs(tmp_path / "d", outs)
    files = sorted((tmp_path / "d").iterdir())
    assert [f.name for f in files] == [f"lookup_{k:02d}.npy" for k in range(12)]
    for k, f in enumerate(files):
        a = np.load(f)
        assert a.dtype == np.float32 and a.shape == (1, 2, 3, 4)
        assert np.array_equal(a, outs[k].numpy())


def test_dump_outputs_samples_large_outputs_within_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4 * 12 * 100)   # 100 elements per file
    g = torch.Generator().manual_seed(5)
    outs = [torch.randn((2, 9, 5, 7), generator=g).bfloat16() for _ in range(12)]
    bench.dump_outputs(tmp_path / "a", outs)
    bench.dump_outputs(tmp_path / "b", outs)
    idx = _sample(outs[0].numel(), 100)
    assert len(np.unique(idx)) == 100
    for k in range(12):
        a = np.load(tmp_path / "a" / f"lookup_{k:02d}.npy")
        assert a.dtype == np.float32 and a.shape == (100,)
        assert np.array_equal(a, outs[k].float().reshape(-1).numpy()[idx])
        assert np.array_equal(a, np.load(tmp_path / "b" / f"lookup_{k:02d}.npy"))
    # several ranks share the budget and name their files apart
    bench.dump_outputs(tmp_path / "r", outs, world=2, rank=1)
    assert np.load(tmp_path / "r" / "rank1_lookup_00.npy").shape == (50,)


def _run_bench(monkeypatch, capsys, *argv):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.parametrize("workload,steps", [("chairs", 6), ("sintel", 4)])
def test_plain_run_dumps_last_step_outputs(monkeypatch, capsys, tmp_path, workload, steps):
    """A plain run: headline fields only, exactly ``--steps`` timed steps, and the
    dumped arrays are the lookups a caller gets from the same inputs (chairs: whole
    outputs; sintel: 109 MB of outputs, so the seeded sample), twice the same."""
    import dexiraft_amd
    res = []
    for d in ("a", "b"):
        res.append(_run_bench(monkeypatch, capsys, "--gpus", "1", "--steps", str(steps),
                              "--warmup", "1", "--clock-warmup-s", "0", "--workload", workload,
                              "--dump-outputs", str(tmp_path / d)))
    r = res[0]
    for key in HEADLINE:
        assert r[key] is not None, key
    assert r["steps"] == steps and r["full"] is False
    assert r["config"]["steps_per_graph"] * int(r["config"]["step_timing"].split(";")[1].split()[0]) \
        == steps
    assert r["value"] == pytest.approx(1e3 / r["ms_per_step"], rel=2e-3)   # ms_per_step: 4 decimals
    assert r["calibration"] is None and r["value_one_step_per_graph"] is None
    assert not any(k in r for k in FULL_ONLY)
    assert res[1]["pair_checksums"] == r["pair_checksums"]

    (_, _), (H, W), B, dtype = bench.WORKLOADS[workload]
    f1, f2, coords = bench.make_inputs(B, H, W, dtype, seed=1234, dev=torch.device("cuda", 0))
    with torch.no_grad():
        blk = dexiraft_amd.CorrBlock(f1, f2, radius=bench.RADIUS)
        want = [blk(c).float().cpu().numpy() for c in coords]
    files = sorted((tmp_path / "a").iterdir())
    assert [f.name for f in files] == [f"lookup_{k:02d}.npy" for k in range(bench.ITERS)]
    assert sum(f.stat().st_size for f in files) <= MAX_DUMP_BYTES
    whole = want[0].nbytes * len(want) <= bench.DUMP_BUDGET_BYTES
    assert whole == (workload == "chairs")
    idx = None if whole else _sample(want[0].size, bench.DUMP_BUDGET_BYTES // (4 * bench.ITERS))
    for k, f in enumerate(files):
        a = np.load(f)
        assert a.dtype == np.float32
        assert np.array_equal(a, want[k] if whole else want[k].reshape(-1)[idx])
        assert np.array_equal(a, np.load(tmp_path / "b" / f.name))


@pytest.mark.gpu
def test_full_run_keeps_the_other_measurements(monkeypatch, capsys):
    r = _run_bench(monkeypatch, capsys, "--gpus", "1", "--steps", "8", "--warmup", "1",
                   "--clock-warmup-s", "0", "--workload", "chairs", "--full", "--cpu-seconds", "0.2")
    assert r["full"] is True and r["steps"] == 8
    for key in HEADLINE + FULL_ONLY + ("calibration", "value_one_step_per_graph"):
        assert r[key] is not None, key
    assert r["roofline"]["avg_launch_us"] > 0 and r["lookup_roofline"]["avg_launch_us"] > 0
    assert r["config"]["kernel_timing"]
