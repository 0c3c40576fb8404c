"""Steer walking flies with the closed-loop tripod CPG: 48 worlds in three groups of 16 with the drives (1, 0.4), (1, 1) and (0.4, 1).
The controller's state lives on the GPU; one control tick = ``cpg.step(20)`` (one controller launch + one 20-step physics launch).
Prints the yaw change per group; ``--film DIR`` also films one world of each group with the batch camera renderer."""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
from flygym_amd import HIPSimulation, make_model
from flygym_amd.controllers import TurningCPG

parser = argparse.ArgumentParser()
parser.add_argument("--seconds", type=float, default=1.0)
parser.add_argument("--film", type=Path, default=None)
args = parser.parse_args()

DRIVES = [(1.0, 0.4), (1.0, 1.0), (0.4, 1.0)]
PER_GROUP = 16
n = PER_GROUP * len(DRIVES)


def yaw(qpos):
    w, x, y, z = qpos[:, 3], qpos[:, 4], qpos[:, 5], qpos[:, 6]
    return torch.atan2(2 * (w * z + x * y), 1 - 2 * (y * y + z * z))


fly, world, cam = make_model()
sim = HIPSimulation(world, n_worlds=n, device=0)
sim.set_leg_adhesion_states(fly.name, np.ones((n, 6), dtype=np.float32))
sim.warmup()
renderer = None
if args.film is not None:
    renderer = sim.set_renderer(cam, worlds=[g * PER_GROUP for g in range(len(DRIVES))], use_gpu_batch_rendering=True)
with TurningCPG(sim, fly.name) as cpg:
    cpg.set_drive(np.repeat(np.array(DRIVES, dtype=np.float32), PER_GROUP, axis=0))
    start = yaw(sim.field("qpos")).clone()
    for _ in range(int(round(args.seconds / (20 * sim.timestep)))):
        cpg.step(20)
        sim.render_as_needed()
    turn = torch.rad2deg(torch.remainder(yaw(sim.field("qpos")) - start + np.pi, 2 * np.pi) - np.pi).reshape(len(DRIVES), PER_GROUP)
    for drive, g, r in zip(DRIVES, turn.cpu().numpy(), cpg.magnitude.reshape(len(DRIVES), PER_GROUP, 6).mean(dim=(1, 2)).cpu().numpy()):
        print(f"drive {drive}: yaw change {g.mean():+7.1f} deg (min {g.min():+.1f}, max {g.max():+.1f}), mean magnitude {r:.3f}")
if renderer is not None:
    for g, drive in enumerate(DRIVES):
        renderer.save_video(g * PER_GROUP, args.film / f"drive_{drive[0]}_{drive[1]}.gif")
    print("films written to", args.film)
