"""Contact-space solve: a step's later eliminations take over the leading pivots they share with the one before
(``dual_eliminate``, ``kDualKeep`` in ``flygym_amd/csrc/nmf_dual.h``) — and not a bit of the step changes.

The engine is built twice into a temporary directory, as it ships and with ``-DNMF_DUAL_NO_RESUME`` (every elimination starts at
ordinal 0; that build's LEGS_ONLY kernels are the machine code from before the change), both with the LEGS_ONLY kernels only
(``-DNMF_TOPO_MASK=1``: the flat-ground and terrain instantiations this test steps, a sixth of the compile time; so the
code object it steps is not the shipped full one, and two instantiations that resume as well are not run here: LEGS_ACTIVE_ONLY and
the tethered LEGS_ONLY kernel — the same ``dual_solve`` text, whose every entry ``scripts/micro/dual_resume_check.cpp`` covers on
the host).  Each build steps,
in a fresh child process of its own, 64 LEGS_ONLY worlds on flat ground through 300 steps of the tripod CPG after the 500-step
settle, and 16 worlds on the blocks terrain through 200; state, accelerations, actuator forces, sensors and the solver's running
counters have to be equal bit for bit.

Eliminations beyond a step's first, from ``stats_sum`` (column 2 = eliminations, column 0 = steps, summed over the stepped region):
there have to be at least 0.30 per step, or the resumed path was hardly exercised.  Measured on the first run: flat 1.529
eliminations per step over 19 200 env-steps, all solved in contact space (0.529 beyond the first), blocks 2.030 over 3 200 (1.03
beyond the first); the bench workload has 0.674 (``profiles/resume_prefix.txt``).  The test took 19 s, builds included.
"""
from __future__ import annotations

import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
FIELDS = ("qpos", "qvel", "qacc", "actuator_force", "sensordata", "stats_sum")

_CHILD = """
import sys
import numpy as np, torch
from flygym_amd import HIPSimulation, make_model
from flygym_amd.controllers import TripodCPG
import flygym_amd.compose as C
from flygym_amd.utils.math import Rotation3D

out = {}
for tag, n, steps in (("flat", 64, 300), ("blocks", 16, 200)):
    fly, world, _ = make_model()
    if tag == "blocks":
        world = C.BlocksTerrainWorld()
        world.add_fly(fly, (0, 0, 0.8), Rotation3D("quat", (1, 0, 0, 0)))
    sim = HIPSimulation(world, n_worlds=n, device=0)
    sim.set_leg_adhesion_states(fly.name, np.ones((n, 6), dtype=np.float32))
    sim.warmup()
    table = TripodCPG(fly.get_actuated_jointdofs_order("position"), sim.timestep).targets(n, 2500, device=sim.device)
    ids = sim.replay_ids(fly.name)
    out[tag + "/sums0"] = sim.field("stats_sum").cpu().numpy().copy()
    for k in range(steps // 50):
        sim.step_replay(table, ids, 50 * k, 50)
    torch.cuda.synchronize()
    for f in %r:
        out[tag + "/" + f] = sim.field(f).cpu().numpy().copy()
np.savez(sys.argv[1], **out)
""" % (FIELDS,)


def _build(tmp: Path):
    from flygym_amd import _native

    libs = {"resume": tmp / "libnmf_resume.so", "restart": tmp / "libnmf_restart.so"}
    procs = [subprocess.Popen(_native.compile_command(libs[k], ["-DNMF_TOPO_MASK=1", *extra]), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
             for k, extra in (("resume", []), ("restart", ["-DNMF_DUAL_NO_RESUME"]))]
    try:
        for p in procs:
            err = p.communicate(timeout=900)[1]      # (a compile takes under a minute)
            assert p.returncode == 0, err[-3000:]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return libs


@pytest.mark.gpu
def test_resumed_eliminations_leave_every_bit_as_it_was(tmp_path):
    libs = _build(tmp_path)
    res = {}
    for key, lib in libs.items():      # one child at a time, each under its own time limit; a child that fails ends the test there
        out = tmp_path / f"{key}.npz"
        r = subprocess.run(["timeout", "-k", "10", "180", sys.executable, "-c", _CHILD, str(out)], capture_output=True, text=True, cwd=ROOT,
                           env=dict(os.environ, NMF_HIP_LIB=str(lib), PYTHONPATH=str(ROOT)))
        assert r.returncode == 0, f"{key} build's child: rc {r.returncode}\n{r.stderr[-3000:]}"
        res[key] = np.load(out)
    a, b = res["resume"], res["restart"]
    for tag in ("flat", "blocks"):
        d = (a[tag + "/stats_sum"].astype(np.int64) - a[tag + "/sums0"].astype(np.int64)).sum(axis=0)
        steps, elims, solved = int(d[0]), int(d[2]), int(d[4])
        print(f"{tag}: {steps} env-steps, {solved} solved in contact space, {elims / steps:.3f} eliminations per step")
        # a step solved in contact space has one elimination; what the counters show beyond that are second and later ones
        later = elims - solved
        assert later >= 0.30 * steps, f"{tag}: {later} eliminations beyond the first on {steps} steps: the resumed path is hardly exercised"
        for f in FIELDS:
            x, y = a[f"{tag}/{f}"], b[f"{tag}/{f}"]
            assert x.dtype == y.dtype and x.shape == y.shape
            assert np.array_equal(x.view(np.uint32) if x.dtype.itemsize == 4 else x, y.view(np.uint32) if y.dtype.itemsize == 4 else y), \
                f"{tag}: {f} differs between the resuming and the restarting build ({int((x != y).sum())} of {x.size} words)"
        assert np.isfinite(a[tag + "/qpos"]).all()
