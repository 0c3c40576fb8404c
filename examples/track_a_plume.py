"""Walk up an odor plume: 256 flies, each in its own plume that a noisy wind blows from a source 10 mm ahead, steered by the
difference between the left and the right antenna's reading.  Everything stays on the GPU: one control tick = one plume tick
(``plume.advance()``), the antennal readings, a few torch operations that turn their asymmetry into the drive of the closed-loop
tripod CPG, and ``cpg.step(20)`` (one controller launch + one 20-step physics launch).  Prints how many flies reached the source
and how many left the arena."""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
from flygym_amd import HIPSimulation, make_model
from flygym_amd.controllers import TurningCPG
from flygym_amd.sensors import OdorPlume

parser = argparse.ArgumentParser()
parser.add_argument("--seconds", type=float, default=2.0)
parser.add_argument("--flies", type=int, default=256)
parser.add_argument("--gain", type=float, default=2.0, help="drive change per unit of antennal asymmetry (L - R) / (L + R)")
args = parser.parse_args()

n = args.flies
STEPS = 20                                   # physics steps per control tick = one plume tick
SOURCE = (10.0, 0.0, 1.0, 1.0)               # x, y, radius (mm), peak
fly, world, _ = make_model()
sim = HIPSimulation(world, n_worlds=n, device=0)
sim.set_leg_adhesion_states(fly.name, np.ones((n, 6), dtype=np.float32))
sim.warmup()
# a 24 mm x 40 mm arena of quarter-millimetre cells; the wind blows from the source towards the flies at 60 mm/s and meanders
plume = OdorPlume(sim, fly.name, grid=(96, 160), cell_size=0.25, origin=(-8.0, -12.0), source=SOURCE, mean_wind=(-60.0, 0.0),
                  wind_tau=0.5, wind_sigma=60.0, diffusivity=1.0, tick_s=STEPS * sim.timestep, seed=1)
with plume, TurningCPG(sim, fly.name) as cpg:
    plume.advance(int(round(0.4 / plume.tick_s)))            # let the plumes reach the flies before they start
    left_arena = torch.zeros(n, dtype=torch.bool, device=sim.device)
    nearest = torch.full((n,), float("inf"), device=sim.device)
    goal = torch.tensor(SOURCE[:2], device=sim.device)
    smelled = torch.zeros(n, dtype=torch.bool, device=sim.device)
    for _ in range(int(round(args.seconds / (STEPS * sim.timestep)))):
        plume.advance()
        odor = plume.get_odor_intensities()[:, 0]                    # (n, 4): palps left / right, antennae left / right
        left, right = odor[:, 2], odor[:, 3]
        turn = args.gain * (left - right) / (left + right + 1e-6)     # > 0: more odor on the left, slow the left legs down
        cpg.drive.copy_(torch.stack([1.0 - turn, 1.0 + turn], dim=1).clamp(0.2, 1.2))
        cpg.step(STEPS)
        left_arena |= plume.out_of_bounds.bool()
        smelled |= left + right > 1e-3
        nearest = torch.minimum(nearest, (sim.field("qpos")[:, :2] - goal).norm(dim=1))
    reached = nearest < SOURCE[2] + 1.0
    walked = sim.field("qpos")[:, 0]
    print(f"{n} flies, {args.seconds:g} s: {int(reached.sum())} reached the source, {int((left_arena & ~reached).sum())} left the arena, "
          f"{int(smelled.sum())} smelled the plume; walked {float(walked.mean()):.1f} mm along x on average (max {float(walked.max()):.1f}), "
          f"nearest approach {float(nearest.min()):.1f} mm, wind now {plume.wind.mean(dim=0).tolist()} mm/s on average")
