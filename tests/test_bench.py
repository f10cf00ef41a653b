"""bench.py on one GPU: what a plain run prints, and that --dump-outputs writes what the timed path computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BENCH = os.path.join(ROOT, "bench.py")


def _env():
    return {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}


def test_bench_refuses_zero_steps():
    """ms_per_step is the time of one of the --steps timed steps: zero of them is refused before anything runs."""
    out = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True, timeout=120, cwd=ROOT, env=_env())
    assert out.returncode == 2 and "--steps must be at least 1" in out.stderr
    assert not [l for l in out.stdout.splitlines() if l.startswith("{")]


@pytest.mark.gpu
@pytest.mark.parametrize("size", [1024, 4096])
def test_plain_bench_line_and_dumped_outputs(size, tmp_path, shipped_defaults):
    """A plain run prints the headline keys and none of what --full adds; --dump-outputs holds the last timed step's output
    plane -- whole at 1024^2, a seeded sample at 4096^2 (16 Mi samples are over the budget) -- and it equals what a plan of
    the same workload computes from the bench's seeded inputs."""
    import torch
    import recfilter_amd as rfa
    import bench
    out = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", "cfg3",
                          "--size", str(size), "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600,
                         cwd=ROOT, env=_env())
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["unit"] == "Mpixels/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["steps"] == 3
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["metric"].startswith("Mpixels/s")
    assert not {"roofline", "kernels_ms", "cpu_baseline", "configs", "value_steady", "sharded_parity"} & set(d)
    assert sorted(os.listdir(tmp_path)) == ["output_plane0.npy"]
    got = np.load(tmp_path / "output_plane0.npy")
    assert got.dtype == np.float32 and got.nbytes <= bench.DUMP_BUDGET_BYTES

    cfg = bench.workload("cfg3", size)
    gen = torch.Generator(device="cuda").manual_seed(1234)
    img = torch.rand(cfg["shape"], generator=gen, device="cuda", dtype=torch.float32)
    with rfa.Plan(cfg["shape"], cfg["scans"], clamped=cfg["clamped"]) as plan:
        assert plan.path_name == d["config"]["path"]
        want = plan.execute([img])[0].reshape(-1).cpu().numpy()
    if size * size * 4 > bench.DUMP_BUDGET_BYTES:
        idx = np.unique(np.random.default_rng(0).integers(0, size * size, bench.DUMP_BUDGET_BYTES // 4))
        assert idx.size < size * size
        want = want[idx]
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-6)
