"""Head stabilization: ALL_BIOLOGICAL flies with position actuators on the two neck dofs that turn the head about the forward and
the lateral axis (``LEVELLING_NECK_DOFS``: in the anatomy's naming the first is the dof named yaw) walk over the blocks terrain under
the closed-loop tripod CPG with piecewise-constant random turning drives.  On the first half of the worlds the inputs of a
``HeadStabilizer`` (leg joint angles, leg contact flags) and the neck angles that would level the head (``ideal_targets`` of the
thorax's attitude) are collected and a small MLP is fitted (``HeadStabilizer.fit``: the form of flygym 1.x's head-stabilization
model).  Then the stabilizer drives the neck, every control tick — ``stab.update()`` + ``cpg.step(20)`` — being one captured graph
that is replayed, beside a twin simulation with the same flies and drives whose neck stays on its passive spring and its
actuators' neutral input.  Prints the RMS world-frame roll and pitch of ``c_head`` on the other half of the worlds for both, and
the thorax's for scale.  Nothing here is a claim: the numbers are what this run measured."""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
import flygym_amd.compose as C
from flygym_amd import HIPSimulation
from flygym_amd import anatomy as A
from flygym_amd.controllers import LEVELLING_NECK_DOFS, HeadStabilizer, TurningCPG
from flygym_amd.utils.math import Rotation3D

parser = argparse.ArgumentParser()
parser.add_argument("--worlds", type=int, default=256)
parser.add_argument("--collect-s", type=float, default=1.0)
parser.add_argument("--test-s", type=float, default=1.0)
parser.add_argument("--drive-s", type=float, default=0.25, help="how long a random drive is held")
parser.add_argument("--epochs", type=int, default=300)
parser.add_argument("--neck-kp", type=float, default=50.0)
parser.add_argument("--seed", type=int, default=0)
args = parser.parse_args()

STEPS = 20
n, half = args.worlds, args.worlds // 2


def build():
    fly = C.Fly(name="nmf")
    fly.add_joints(A.Skeleton(axis_order=A.AxisOrder.YAW_PITCH_ROLL, joint_preset=A.JointPreset.ALL_BIOLOGICAL), neutral_pose=C.KinematicPosePreset.NEUTRAL)
    legs = A.Skeleton(axis_order=A.AxisOrder.YAW_PITCH_ROLL, joint_preset=A.JointPreset.LEGS_ONLY)
    fly.add_actuators(legs.get_actuated_dofs_from_preset("legs_active_only"), C.ActuatorType.POSITION, kp=50.0,
                      neutral_input=C.KinematicPosePreset.NEUTRAL)
    fly.add_actuators([A.JointDOF.from_name(d) for d in LEVELLING_NECK_DOFS], C.ActuatorType.POSITION, kp=args.neck_kp)
    fly.add_leg_adhesion()
    world = C.BlocksTerrainWorld()
    world.add_fly(fly, (0.3, 0.2, 1.0), Rotation3D("quat", (1, 0, 0, 0)))
    sim = HIPSimulation(world, n_worlds=n, device=0)
    sim.set_leg_adhesion_states(fly.name, np.ones((n, 6), dtype=np.float32))
    sim.warmup()
    return fly, sim


fly, sim = build()              # the neck will be driven
_, twin = build()               # the same flies and drives, the neck left alone
tick_s = STEPS * sim.timestep
hold = max(1, int(round(args.drive_s / tick_s)))
rng = np.random.default_rng(args.seed)
segs = [s.name for s in fly.get_bodysegs_order()]
head, thorax = segs.index("c_head"), segs.index(fly.root_segment.name)
print(f"seed {args.seed}: 2 x {n} ALL_BIOLOGICAL flies on the blocks terrain, control tick {tick_s * 1e3:.1f} ms, a new random drive every {hold} ticks")


def attitude(s, seg):
    """(n, 2): world-frame roll and pitch of a segment."""
    return -HeadStabilizer.ideal_targets(s.field("seg_xquat").view(n, s.model.nseg, 4)[:, seg])


with TurningCPG(sim, fly.name, table_steps=STEPS) as cpg, TurningCPG(twin, fly.name, table_steps=STEPS) as cpg_twin:
    def new_drive():
        drive = torch.as_tensor(rng.uniform(0.4, 1.2, (n, 2)).astype(np.float32))
        cpg.set_drive(drive)
        cpg_twin.set_drive(drive)

    # ---- collected on the first half of the worlds (both simulations take the same steps: they stay twins)
    T = int(round(args.collect_s / tick_s))
    inputs, targets = [], []
    for k in range(T):
        if k % hold == 0:
            new_drive()
        cpg.step(STEPS)
        cpg_twin.step(STEPS)
        inputs.append(HeadStabilizer.collect_inputs(sim, fly.name)[:half].clone())
        targets.append(HeadStabilizer.ideal_targets(sim.field("seg_xquat").view(n, sim.model.nseg, 4)[:half, thorax]).clone())
    torch.cuda.synchronize()
    same = all(torch.equal(sim.field(k), twin.field(k)) for k in ("qpos", "qvel"))
    X, Y = torch.cat(inputs).cpu(), torch.cat(targets).cpu()
    layers, mean, std = HeadStabilizer.fit(X, Y, epochs=args.epochs, seed=args.seed)
    print(f"collected {tuple(X.shape)} inputs on worlds 0..{half - 1} over {T} ticks (the twins are {'identical' if same else 'NOT identical'}); "
          f"targets' RMS roll {float(Y[:, 0].square().mean().sqrt()):.4f} rad, pitch {float(Y[:, 1].square().mean().sqrt()):.4f} rad")

    # ---- the other half is scored: the stabilizer in a captured tick, the twin without it
    with HeadStabilizer(sim, fly.name, layers, input_mean=mean, input_std=std, output_dofs=LEVELLING_NECK_DOFS) as stab:
        stab.update()
        torch.cuda.synchronize()
        pred = stab.output[:half].cpu()
        now = HeadStabilizer.ideal_targets(sim.field("seg_xquat").view(n, sim.model.nseg, 4)[:half, thorax]).cpu()
        print(f"fitted 48 -> 32 -> 32 -> 2 over {args.epochs} epochs; residual RMS on the last collected tick: roll "
              f"{float((pred - now)[:, 0].square().mean().sqrt()):.4f} rad, pitch {float((pred - now)[:, 1].square().mean().sqrt()):.4f} rad")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            stab.update()
            cpg.step(STEPS)
        sums = {name: torch.zeros((n, 2), dtype=torch.float64, device=sim.device) for name in ("head", "head_twin", "thorax", "thorax_twin")}
        ticks = int(round(args.test_s / tick_s))
        for k in range(ticks):
            if k % hold == 0:
                new_drive()
            graph.replay()
            cpg_twin.step(STEPS)
            for name, s, seg in (("head", sim, head), ("head_twin", twin, head), ("thorax", sim, thorax), ("thorax_twin", twin, thorax)):
                sums[name] += attitude(s, seg).double() ** 2
        torch.cuda.synchronize()
        rms = {name: torch.sqrt(v[half:].mean(dim=0) / ticks).cpu().numpy() for name, v in sums.items()}
        finite = bool(torch.isfinite(sim.field("qpos")).all() and torch.isfinite(twin.field("qpos")).all())
        print(f"scored on worlds {half}..{n - 1} over {args.test_s:g} s ({ticks} replays of one graph); all finite: {finite}")
        for name, label in (("head", "c_head, stabilized"), ("head_twin", "c_head, neck left alone"), ("thorax", "c_thorax, stabilized run"),
                            ("thorax_twin", "c_thorax, twin run")):
            print(f"  RMS world-frame roll / pitch of {label:26s}: {rms[name][0]:.4f} / {rms[name][1]:.4f} rad "
                  f"({np.degrees(rms[name][0]):.2f} / {np.degrees(rms[name][1]):.2f} deg)")
