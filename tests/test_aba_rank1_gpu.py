"""Leg-chain kernels: the rank-1 downdates of the fused smooth solve's two articulated-body chains (legs, root, and the Euler
factors' ``aba_root_factor``) run on the matrix pipe (``kAbaRank1Mfma`` in ``flygym_amd/csrc/nmf_step_lds.h``,
``grp8_rank1_mfma`` in ``nmf_device.h``) — and not a bit of a step changes.

The engine is built twice into a temporary directory, as it ships and with ``-DNMF_ABA_RANK1_VALU`` (six group broadcasts and
three packed multiply-adds per downdate; that build's machine code is the one from before the change), both with the two
leg-chain families only (``-DNMF_TOPO_MASK=3``), in parallel.  Each build steps, in a fresh child process of its own:

* ``flat`` — 64 LEGS_ONLY worlds on flat ground, 60 steps straight from the reset (the fly falls: steps without a contact), then
  100 steps of the tripod CPG in 50-step launches (steps solved in contact space);
* ``blocks`` — 16 worlds on the blocks terrain, 100 steps (the terrain instantiation);
* ``tethered`` — 16 tethered LEGS_ONLY worlds, 50 steps (the weld instantiation, primal loop);
* ``active`` — 16 LEGS_ACTIVE_ONLY worlds on flat ground, 100 steps.

State, accelerations, actuator forces, sensors, segment poses and the solver's counters are compared as 32-bit words.
"""
from __future__ import annotations

import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
FIELDS = ("qpos", "qvel", "qacc", "actuator_force", "sensordata", "seg_xpos", "seg_xquat", "stats_sum")
CASES = ("flat", "blocks", "tethered", "active")

_CHILD = """
import sys
import numpy as np, torch
from flygym_amd import HIPSimulation, make_model
from flygym_amd.controllers import TripodCPG
import flygym_amd.compose as C
from flygym_amd.utils.math import Rotation3D

upright = Rotation3D("quat", (1, 0, 0, 0))
out = {}
# case: (worlds, steps from the reset in one launch, CPG steps in 50-step launches)
for tag, n, free, steps in (("flat", 64, 60, 100), ("blocks", 16, 0, 100), ("tethered", 16, 0, 50), ("active", 16, 0, 100)):
    fly, world, _ = make_model(joints_preset="legs_active_only" if tag == "active" else "legs_only")
    if tag == "blocks":
        world = C.BlocksTerrainWorld(); world.add_fly(fly, (0, 0, 0.8), upright)
    if tag == "tethered":
        world = C.TetheredWorld(); world.add_fly(fly, (0, 0, 1.5), upright)
    sim = HIPSimulation(world, n_worlds=n, device=0)
    sim.set_leg_adhesion_states(fly.name, np.ones((n, 6), dtype=np.float32))
    if free:
        sim.step(free)
    table = TripodCPG(fly.get_actuated_jointdofs_order("position"), sim.timestep).targets(n, 2500, device=sim.device)
    ids = sim.replay_ids(fly.name)
    for k in range(steps // 50):
        sim.step_replay(table, ids, 50 * k, 50)
    torch.cuda.synchronize()
    info = sim.batch_info()
    out[tag + "/info"] = np.array([info["kernel_family"], info["terrain_kernel"], info["tether_kernel"]])
    for f in %r:
        out[tag + "/" + f] = sim.field(f).cpu().numpy().copy()
np.savez(sys.argv[1], **out)
""" % (FIELDS,)


def _build(tmp: Path):
    from flygym_amd import _native

    libs = {"mfma": tmp / "libnmf_mfma.so", "valu": tmp / "libnmf_valu.so"}
    procs = [subprocess.Popen(_native.compile_command(libs[k], ["-DNMF_TOPO_MASK=3", *extra]), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
             for k, extra in (("mfma", []), ("valu", ["-DNMF_ABA_RANK1_VALU"]))]
    try:
        for p in procs:
            err = p.communicate(timeout=900)[1]      # (a compile takes about a minute)
            assert p.returncode == 0, err[-3000:]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return libs


def _words(x):
    return x.view(np.uint32) if x.dtype.itemsize == 4 else x


@pytest.mark.gpu
def test_matrix_pipe_downdates_leave_every_bit_as_it_was(tmp_path):
    libs = _build(tmp_path)
    res = {}
    for key, lib in libs.items():      # one child at a time, each under its own time limit; a child that fails ends the test there
        out = tmp_path / f"{key}.npz"
        r = subprocess.run(["timeout", "-k", "10", "180", sys.executable, "-c", _CHILD, str(out)], capture_output=True, text=True, cwd=ROOT,
                           env=dict(os.environ, NMF_HIP_LIB=str(lib), PYTHONPATH=str(ROOT)))
        assert r.returncode == 0, f"{key} build's child: rc {r.returncode}\n{r.stderr[-3000:]}"
        res[key] = np.load(out)
    a, b = res["mfma"], res["valu"]
    # the instantiations the cases are meant to run: (kernel_family, terrain_kernel, tether_kernel)
    kernels = {"flat": (0, 0, 0), "blocks": (0, 1, 0), "tethered": (0, 0, 1), "active": (1, 0, 0)}
    for tag in CASES:
        for r in (a, b):
            assert tuple(r[tag + "/info"]) == kernels[tag], f"{tag}: runs kernel {tuple(r[tag + '/info'])}"
        for f in FIELDS:
            x, y = a[f"{tag}/{f}"], b[f"{tag}/{f}"]
            assert x.dtype == y.dtype and x.shape == y.shape
            assert np.array_equal(_words(x), _words(y)), \
                f"{tag}: {f} differs between the matrix-pipe and the vector-pipe build ({int((_words(x) != _words(y)).sum())} of {x.size} words)"
        assert np.isfinite(a[tag + "/qpos"]).all()
    # flat: steps without a contact (stats_sum column 14) and steps solved in contact space (column 4)
    sums = a["flat/stats_sum"].astype(np.int64).sum(axis=0)
    print(f"flat: {int(sums[0])} env-steps, {int(sums[14])} without a contact, {int(sums[4])} solved in contact space")
    assert sums[0] == 64 * 160 and sums[14] > 0 and sums[4] > 0, sums.tolist()
