"""The step's fixed cost around its stages (``kStepCursor`` / ``kInertiaInKin`` in ``flygym_amd/csrc/nmf_step_lds.h``): the step
loop carries the control table's row from step to step instead of taking two modulos per step, and the ``stage_kinematics`` of
the leg-chain kernels of flat and tethered worlds requests the bodies' inertial constants at its entry and builds ``Ib`` /
``Isym`` itself — and not a bit of a step changes.

The engine is built twice into a temporary directory, as it ships and with ``-DNMF_STEP_FIXED_OLD`` (the step loop's modulos,
the inertia stage behind the kinematics call), both with the two leg-chain families only (``-DNMF_TOPO_MASK=3``), in parallel.
Each build steps, in a fresh child process of its own, the smallest shapes at which every changed path runs:

* ``flat`` — 64 LEGS_ONLY worlds on flat ground, 60 steps straight from the reset, then 100 steps of the tripod CPG in 50-step
  launches;
* ``blocks`` — 16 worlds on the blocks terrain, 100 steps (the terrain instantiation);
* ``tethered`` — 16 tethered worlds, 50 steps (the weld instantiation);
* ``active`` — 16 LEGS_ACTIVE_ONLY worlds, 100 steps (25 bodies: the lanes without a body of the in-stage inertia);
* ``chunk`` / ``plain`` — 288 worlds at one fly per CU, a settle and one 50-step launch on the chunked schedule (every item
  takes its own modulo at its first step) against the same worlds on the plain schedule;
* ``wrap*`` — what the row cursor can get wrong.  16 flat worlds replay a table of 70 rows: a 50-step launch from ``start`` 45
  (the wrap falls inside the launch), from 69 (the launch starts on the table's last row) and from 150 (beyond the table), then
  a launch of 1 step and one of 3 steps from row 69; and 288 worlds at one fly per CU from 45, where the chunks' boundaries
  fall beside the wrap;
* ``ring1`` / ``ring5`` — one 50-step launch that records every step / every fifth step: the observation ring word for word.

State, accelerations, actuator forces, sensors, segment poses and the solver's counters are compared as 32-bit words.

A second test does the same for one ALL_BIOLOGICAL case (8 worlds, 50 steps from row 45 of a 70-row table: the same loop in a
kernel of another family) on full-library builds.  Two full builds take about three minutes each, far over this module's minute,
so it runs only where ``NMF_STEP_FIXED_FULL_DIR`` names a directory to build them into (or that holds them already:
``libnmf_shipped.so`` and ``libnmf_old.so``) and is skipped with that reason otherwise.

Measured on the first run: the leg-chain test took 25 s, builds included (flat case: 7678 of its 10 240 env-steps without a
contact, 2562 solved in contact space); the full-library test, on prebuilt libraries, 6 s.
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
KERNELS = {"flat": (0, 0, 0), "blocks": (0, 1, 0), "tethered": (0, 0, 1), "active": (1, 0, 0), "chunk": (0, 0, 0), "plain": (0, 0, 0)}
WRAPS = ("wrap45", "wrap69", "wrap150", "wrap1", "wrap3", "wrapchunk")

_CHILD = """
import sys
import numpy as np, torch
from flygym_amd import HIPSimulation, make_model
from flygym_amd.controllers import TripodCPG
import flygym_amd.compose as C
from flygym_amd.utils.math import Rotation3D

FIELDS = %r
upright = Rotation3D("quat", (1, 0, 0, 0))
out = {}

def snap(sim, tag):
    torch.cuda.synchronize()
    for f in FIELDS:
        out[tag + "/" + f] = sim.field(f).cpu().numpy().copy()

def make(n, preset="legs_only", kind="flat", opts={}):
    fly, world, _ = make_model(joints_preset=preset)
    if kind == "blocks":
        world = C.BlocksTerrainWorld(); world.add_fly(fly, (0, 0, 0.8), upright)
    if kind == "tethered":
        world = C.TetheredWorld(); world.add_fly(fly, (0, 0, 1.5), upright)
    sim = HIPSimulation(world, n_worlds=n, device=0, _options=opts)
    sim.set_leg_adhesion_states(fly.name, np.ones((n, 6), dtype=np.float32))
    cpg = TripodCPG(fly.get_actuated_jointdofs_order("position"), sim.timestep)
    return fly, sim, cpg, sim.replay_ids(fly.name)

def info_of(sim):
    info = sim.batch_info()
    return np.array([info["chunked"], info["resident_workgroups"], info["kernel_family"], info["terrain_kernel"], info["tether_kernel"]])

if sys.argv[2] == "legs":
    # case: (worlds, steps from the reset in one launch, CPG steps in 50-step launches, create options)
    for tag, n, free, steps, opts in (("flat", 64, 60, 100, {}), ("blocks", 16, 0, 100, {}), ("tethered", 16, 0, 50, {}), ("active", 16, 0, 100, {}),
                                      ("chunk", 288, 500, 50, dict(flies_per_cu=1)), ("plain", 288, 500, 50, dict(flies_per_cu=1, sched="plain"))):
        fly, sim, cpg, ids = make(n, "legs_active_only" if tag == "active" else "legs_only", tag, opts)
        if free:
            sim.step(free)
        table = cpg.targets(n, 2500, device=sim.device)
        for k in range(steps // 50):
            sim.step_replay(table, ids, 50 * k, 50)
        out[tag + "/info"] = info_of(sim)
        snap(sim, tag)
    # the cursor: a 70-row table, launches that wrap inside, start on the last row, start beyond the table; 1 and 3 steps
    fly, sim, cpg, ids = make(16)
    sim.step(60)
    table = cpg.targets(16, 70, device=sim.device).contiguous()
    for tag, start, steps in (("wrap45", 45, 50), ("wrap69", 69, 50), ("wrap150", 150, 50), ("wrap1", 69, 1), ("wrap3", 69, 3)):
        sim.step_replay(table, ids, start, steps)
        snap(sim, tag)
    # the observation ring, every step and every fifth
    for k in (1, 5):
        ring = sim.step_replay(table, ids, 45, 50, record_every=k)
        torch.cuda.synchronize()
        out["ring%%d/ring" %% k] = ring.cpu().numpy().copy()
        snap(sim, "ring%%d" %% k)
    fly, sim, cpg, ids = make(288, opts=dict(flies_per_cu=1))
    sim.step(500)
    sim.step_replay(cpg.targets(288, 70, device=sim.device).contiguous(), ids, 45, 50)
    out["wrapchunk/info"] = info_of(sim)
    snap(sim, "wrapchunk")
else:
    fly, sim, cpg, ids = make(8, "all_biological")
    sim.step_replay(cpg.targets(8, 70, device=sim.device).contiguous(), ids, 45, 50)
    out["bio/info"] = info_of(sim)
    snap(sim, "bio")
np.savez(sys.argv[1], **out)
""" % (FIELDS,)


def _build(libs: dict, flags: dict):
    from flygym_amd import _native

    todo = [k for k in libs if not libs[k].exists()]
    procs = {k: subprocess.Popen(_native.compile_command(libs[k], flags[k]), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True) for k in todo}
    try:
        for p in procs.values():
            err = p.communicate(timeout=1500)[1]
            assert p.returncode == 0, err[-3000:]
    finally:
        for p in procs.values():
            if p.poll() is None:
                p.kill()
    return libs


def _run(libs: dict, tmp: Path, mode: str):
    res = {}
    for key, lib in libs.items():      # one child at a time, each under its own time limit; a child that fails ends the test there
        out = tmp / f"{key}_{mode}.npz"
        r = subprocess.run(["timeout", "-k", "10", "180", sys.executable, "-c", _CHILD, str(out), mode], capture_output=True, text=True, cwd=ROOT,
                           env=dict(os.environ, NMF_HIP_LIB=str(lib), PYTHONPATH=str(ROOT)))
        assert r.returncode == 0, f"{key} build's child: rc {r.returncode}\n{r.stderr[-3000:]}"
        res[key] = np.load(out)
    return res["shipped"], res["old"]


def _words(x):
    return x.view(np.uint32) if x.dtype.itemsize == 4 else x


def _same(a, b, tag, fields=FIELDS):
    for f in fields:
        x, y = a[f"{tag}/{f}"], b[f"{tag}/{f}"]
        assert x.dtype == y.dtype and x.shape == y.shape
        assert np.array_equal(_words(x), _words(y)), \
            f"{tag}: {f} differs between the shipped and the -DNMF_STEP_FIXED_OLD build ({int((_words(x) != _words(y)).sum())} of {x.size} words)"
    assert np.isfinite(a[tag + "/qpos"]).all()


@pytest.mark.gpu
def test_step_fixed_cost_leaves_every_bit_as_it_was(tmp_path):
    libs = _build({"shipped": tmp_path / "libnmf_shipped.so", "old": tmp_path / "libnmf_old.so"},
                  {"shipped": ["-DNMF_TOPO_MASK=3"], "old": ["-DNMF_TOPO_MASK=3", "-DNMF_STEP_FIXED_OLD"]})
    a, b = _run(libs, tmp_path, "legs")
    for tag, kernel in KERNELS.items():
        assert tuple(a[tag + "/info"][2:]) == kernel, f"{tag}: runs kernel {tuple(a[tag + '/info'][2:])}"
        _same(a, b, tag)
    for tag in WRAPS:
        _same(a, b, tag)
    for tag in ("ring1", "ring5"):
        _same(a, b, tag, FIELDS + ("ring",))
    assert a["ring1/ring"].shape[0] == 50 and a["ring5/ring"].shape[0] == 10 and np.isfinite(a["ring1/ring"]).all()
    sums = a["flat/stats_sum"].astype(np.int64).sum(axis=0)
    print(f"flat: {int(sums[0])} env-steps, {int(sums[14])} without a contact, {int(sums[4])} solved in contact space")
    assert sums[0] == 64 * 160 and sums[14] > 0 and sums[4] > 0, sums.tolist()
    # the wrapped launches did step and did follow the table: a launch beyond the table replays rows 10.., not rows 45.. again
    assert not np.array_equal(_words(a["wrap45/qpos"]), _words(a["wrap69/qpos"]))
    # chunked schedule: fewer workgroups than worlds, every item of a world takes its row by its own modulo; the same bits as the plain one
    for r in (a, b):
        for tag in ("chunk", "wrapchunk"):
            assert int(r[tag + "/info"][0]) == 1 and int(r[tag + "/info"][1]) < 288, r[tag + "/info"].tolist()
        assert int(r["plain/info"][0]) == 0
        for f in FIELDS:
            assert np.array_equal(_words(r[f"chunk/{f}"]), _words(r[f"plain/{f}"])), f"{f} differs between the chunked and the plain schedule"


@pytest.mark.gpu
def test_step_fixed_cost_full_library_all_biological(tmp_path):
    where = os.environ.get("NMF_STEP_FIXED_FULL_DIR")
    if not where:
        reason = "two full-library builds take about three minutes each, over this module's one-minute budget: set NMF_STEP_FIXED_FULL_DIR to run it"
        print(reason)
        pytest.skip(reason)
    d = Path(where)
    d.mkdir(parents=True, exist_ok=True)
    libs = _build({"shipped": d / "libnmf_shipped.so", "old": d / "libnmf_old.so"}, {"shipped": [], "old": ["-DNMF_STEP_FIXED_OLD"]})
    a, b = _run(libs, tmp_path, "bio")
    print("ALL_BIOLOGICAL runs kernel family", int(a["bio/info"][2]))
    _same(a, b, "bio")
    assert a["bio/stats_sum"].astype(np.int64).sum(axis=0)[0] == 8 * 50
