"""What walking flies do to the quantities ``WalkingTask`` thresholds, measured on the GPU: the numbers its defaults rest on
(recorded by hand in profiles/task_summary.md).

--worlds flies with random drives in 0.4..1.2 walk under ``TurningCPG`` for --ticks control ticks of 20 steps on flat ground and on
the blocks terrain; per tick the script reads, in torch, the root segment's height and ``up_z = 1 - 2 (qx^2 + qy^2)``, the six leg
contact flags (``controllers._leg_contact_flags`` with the default thresholds) and ``|force * qvel|`` of the 42 leg actuators, and
keeps their ranges, the longest run of ticks with no flag set and the quantiles of the power terms.  Then every world is reset to
the keyframe and the ticks until its first flag are counted.  Last, the 41 tumbling states of tests/tumbling_states.py fall for
--ticks ticks on flat ground: what ``up_z`` and the height do when a fly does not walk.  Needs an MI355X: no fallback."""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np
import torch
from flygym_amd import HIPSimulation, make_model
from flygym_amd.controllers import TurningCPG, _leg_contact_flags
from flygym_amd.tasks import WalkingTask

parser = argparse.ArgumentParser()
parser.add_argument("--worlds", type=int, default=256)
parser.add_argument("--ticks", type=int, default=150)
parser.add_argument("--settle-ticks", type=int, default=25)
parser.add_argument("--out", type=Path, default=None)
args = parser.parse_args()
if not torch.cuda.is_available():
    sys.exit("task_survey.py measures on the GPU and found none")
STEPS = 20


def blocks_world():
    import flygym_amd.compose as C
    from flygym_amd import anatomy as A
    from flygym_amd.utils.math import Rotation3D

    fly = C.Fly(name="nmf")
    sk = A.Skeleton(axis_order=A.AxisOrder.YAW_PITCH_ROLL, joint_preset=A.JointPreset.LEGS_ONLY)
    fly.add_joints(sk, neutral_pose=C.KinematicPosePreset.NEUTRAL)
    fly.add_actuators(sk.get_actuated_dofs_from_preset("legs_active_only"), C.ActuatorType.POSITION, kp=50.0,
                      neutral_input=C.KinematicPosePreset.NEUTRAL)
    fly.add_leg_adhesion()
    world = C.BlocksTerrainWorld()
    world.add_fly(fly, (0.3, 0.2, 0.8), Rotation3D("quat", (1, 0, 0, 0)))
    return fly, world


class Probe:
    """The thresholded quantities of one batch, read in torch."""

    def __init__(self, sim, fly):
        self.sim, n = sim, sim.n_worlds
        self.task = WalkingTask(sim, fly.name)
        dev = sim.device
        ids = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int64), device=dev)
        self.act, self.act_dof = ids(self.task._act), ids(6 + self.task._act_dof)
        self.thr2 = torch.as_tensor(self.task.thr2, device=dev)
        self.root = self.task.root_seg
        self.nseg = sim.model.nseg

    def read(self):
        sim, n = self.sim, self.sim.n_worlds
        z = sim.field("seg_xpos").view(n, self.nseg, 3)[:, self.root, 2]
        q = sim.field("seg_xquat").view(n, self.nseg, 4)[:, self.root]
        up_z = 1 - 2 * (q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2])
        flags = _leg_contact_flags(torch, sim.field("sensordata"), self.thr2)
        power = (sim.field("actuator_force")[:, self.act] * sim.field("qvel")[:, self.act_dof]).abs()
        return z.clone(), up_z, flags.sum(dim=1), power


def rng_range(t):
    return [float(t.min()), float(t.max())]


def walk(name, fly, world):
    n = args.worlds
    sim = HIPSimulation(world, n_worlds=n, device=0)
    sim.set_leg_adhesion_states(fly.name, np.ones((n, 6), dtype=np.float32))
    sim.warmup()
    probe = Probe(sim, fly)
    out = {}
    with TurningCPG(sim, fly.name, table_steps=32) as cpg:
        drive = torch.as_tensor(np.random.default_rng(2).uniform(0.4, 1.2, (n, 2)).astype(np.float32), device=sim.device)
        cpg.set_drive(drive)
        for _ in range(args.settle_ticks):
            cpg.step(STEPS)
        zs, ups, powers, nflags = [], [], [], []
        run = torch.zeros(n, dtype=torch.int64, device=sim.device)
        longest = torch.zeros_like(run)
        for _ in range(args.ticks):
            cpg.step(STEPS)
            z, up_z, k, power = probe.read()
            zs.append(z); ups.append(up_z); powers.append(power); nflags.append(k)
            run = torch.where(k == 0, run + 1, torch.zeros_like(run))
            longest = torch.maximum(longest, run)
        z, up, p, k = torch.stack(zs), torch.stack(ups), torch.stack(powers).flatten(), torch.stack(nflags)
        qs = torch.tensor([0.5, 0.9, 0.99, 0.999, 0.9999], device=sim.device)
        sample = p[torch.randperm(p.numel(), device=sim.device)[:4_000_000]] if p.numel() > 4_000_000 else p
        out["walking"] = dict(ticks=args.ticks, finite=bool(torch.isfinite(z).all() and torch.isfinite(p).all()), z=rng_range(z),
                              up_z=rng_range(up), tilt_deg_max=float(torch.rad2deg(torch.acos(up.min().clamp(-1, 1)))),
                              flags_set=rng_range(k), ticks_without_flag_share=float((k == 0).float().mean()),
                              longest_run_without_flag=int(longest.max()),
                              power_quantiles=dict(zip(map(str, qs.tolist()), torch.quantile(sample, qs).tolist())), power_max=float(p.max()),
                              power_sum_per_tick=rng_range(torch.stack(powers).sum(dim=2)))
        # from the keyframe: the drop, the landing, the first stance
        sim.reset()
        cpg.reset()
        cpg.set_drive(drive)
        first = torch.full((n,), -1, dtype=torch.int64, device=sim.device)
        zs, ups = [], []
        for t in range(40):
            cpg.step(STEPS)
            z, up_z, k, _ = probe.read()
            zs.append(z); ups.append(up_z)
            first = torch.where((first < 0) & (k > 0), torch.full_like(first, t + 1), first)
        z, up = torch.stack(zs), torch.stack(ups)
        out["from_keyframe"] = dict(first_tick_with_flag=rng_range(first), z_first_40_ticks=rng_range(z), up_z_first_40_ticks=rng_range(up),
                                    z_per_tick_min=[round(float(v), 4) for v in z.min(dim=1).values[:12]],
                                    z_per_tick_max=[round(float(v), 4) for v in z.max(dim=1).values[:12]])
    probe.task.close()
    sim.close() if hasattr(sim, "close") else None
    print(name, json.dumps(out))
    return out


def tumble():
    import tumbling_states as ts

    fly, world, _ = make_model()
    sim = HIPSimulation(world, n_worlds=ts.N_STATES, device=0)
    qpos, qvel, ctrl = ts.states(sim.model, 11)
    sim.reset()
    for name, a in (("qpos", qpos), ("qvel", qvel), ("ctrl", ctrl)):
        sim.field(name).copy_(torch.as_tensor(a.astype(np.float32), device=sim.device))
    probe = Probe(sim, fly)
    zs, ups = [], []
    for _ in range(args.ticks):
        sim.step(STEPS)
        z, up_z, _, _ = probe.read()
        zs.append(z); ups.append(up_z)
    z, up = torch.stack(zs), torch.stack(ups)
    ok = torch.isfinite(z) & torch.isfinite(up)
    cos70 = float(np.cos(np.deg2rad(70.0)))
    below = (up < cos70) & ok
    run = torch.zeros(ts.N_STATES, dtype=torch.int64, device=sim.device)
    longest = torch.zeros_like(run)
    for t in range(args.ticks):
        run = torch.where(below[t], run + 1, torch.zeros_like(run))
        longest = torch.maximum(longest, run)
    tiers = np.array([ts.tier(w) for w in range(ts.N_STATES)])
    out = dict(ticks=args.ticks, worlds_not_finite=int((~ok).any(dim=0).sum()), up_z=rng_range(up[ok]), z=rng_range(z[ok]),
               worlds_with_up_z_below_cos70_for_5_ticks=int((longest >= 5).sum()), longest_run_below_cos70=longest.tolist(),
               z_last_tick_by_tier={str(t): rng_range(z[-1][torch.as_tensor(tiers == t, device=sim.device) & ok[-1]]) for t in ts.TIERS
                                    if bool((torch.as_tensor(tiers == t, device=sim.device) & ok[-1]).any())},
               up_z_last_tick=rng_range(up[-1][ok[-1]]))
    probe.task.close()
    print("tumbling", json.dumps(out))
    return out


result = dict(worlds=args.worlds, steps_per_tick=STEPS)
fly, world, _ = make_model()
result["flat"] = walk("flat", fly, world)
result["blocks"] = walk("blocks", *blocks_world())
result["tumbling"] = tumble()
print(json.dumps(result))
if args.out is not None:
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(result, indent=1) + "\n")
