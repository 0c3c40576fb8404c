"""bench.py's plain run and ``--dump-outputs``: the CPU side of the dump (budget, seeded world sample) and one plain run of
the headline workload on the GPU (exactly ``--steps`` timed steps, no ``--full`` extras, the last step's outputs on disk)."""
import importlib
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


def _bench():
    sys.path.insert(0, str(ROOT))
    return importlib.import_module("bench")


def test_plain_run_arguments():
    bench = _bench()
    args = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert not args.full and args.repeats == 1 and args.dump_outputs is None
    args = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert args.full and args.dump_outputs == "out"


def test_dump_outputs_keeps_one_seeded_sample_of_worlds_within_the_budget(tmp_path):
    import torch

    bench = _bench()
    n = 1000
    world = torch.arange(n, dtype=torch.float32)
    arrays = {"qpos": (world[:, None] * 100 + torch.arange(73, dtype=torch.float32), 0),
              "observations": (world[None, :, None].expand(5, n, 270).contiguous(), 1),
              "site_xpos": (torch.zeros(n, 0), 0)}
    total = 4 * (n * 73 + 5 * n * 270)
    bench.dump_outputs(tmp_path / "all", arrays, n, budget=total)
    assert np.array_equal(np.load(tmp_path / "all" / "qpos.npy"), arrays["qpos"][0].numpy())
    assert not (tmp_path / "all" / "site_xpos.npy").exists()                 # nothing to compare: not written

    for run in ("a", "b"):
        bench.dump_outputs(tmp_path / run, arrays, n, budget=total // 3)
    q, o = np.load(tmp_path / "a" / "qpos.npy"), np.load(tmp_path / "a" / "observations.npy")
    assert q.dtype == o.dtype == np.float32
    assert 4 * (q.size + o.size) <= total // 3 and q.shape[0] == o.shape[1] >= n // 3 - 1
    ids = q[:, 0] / 100
    assert np.all(np.diff(ids) > 0) and np.array_equal(ids, o[0, :, 0])     # the same worlds, in world order
    for name in ("qpos", "observations"):                                    # the same sample from run to run
        assert np.array_equal(np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy"))


@pytest.mark.gpu
def test_plain_bench_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    steps = 100
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "50",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')]
    assert r.returncode == 0 and len(lines) == 1, r.stdout[-2000:] + r.stderr[-2000:]
    d = json.loads(lines[0])
    assert d["valid"] and d["unit"] == "env-steps/s" and d["higher_is_better"] and d["dtype"] == "f32"
    c = d["config"]
    assert d["steps"] == steps and c["repeats"] == 1 and c["timed_steps_total"] == steps
    assert d["ms_per_step"] == pytest.approx(c["elapsed_s"]["total"] * 1e3 / steps)
    assert d["value"] == pytest.approx(c["total_worlds"] * steps / c["elapsed_s"]["total"])
    assert "cpu_baseline" not in d and "other_configs" not in d and d["roofline"]["counters"] == "replayed"
    files = {p.stem: np.load(p) for p in tmp_path.glob("*.npy")}
    assert {"qpos", "qvel", "qacc", "actuator_force", "sensordata", "seg_xpos", "seg_xquat"} <= set(files) <= set(_bench().DUMP_FIELDS)
    assert sum(p.stat().st_size for p in tmp_path.glob("*.npy")) <= 64 * 10**6
    assert files["qpos"].shape == (4096, 73) and files["qvel"].shape == (4096, 72) and files["sensordata"].shape == (4096, 96)
    for name, a in files.items():
        assert a.dtype == np.float32 and np.isfinite(a).all(), name
