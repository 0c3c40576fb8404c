"""Follow a dark target through an odor plume: 64 flies, each with a black sphere that circles it at 8 mm and a plume that a noisy
wind blows at it, steered by its eyes and its antennae.  Everything stays on the GPU: one control tick is ``plume.advance()`` -> the
antennal readings -> ``eyes.render_into`` -> ``steer.update(out=cpg.drive)`` (one launch: readings to drive) -> ``cpg.step(20)``,
captured once as a graph and replayed; between replays two torch operations move every fly's sphere in place.  Prints how many
flies kept the target in view."""
import argparse
import math
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
from flygym_amd import HIPSimulation, make_model
from flygym_amd.controllers import SensorySteering, TurningCPG
from flygym_amd.sensors import OdorPlume
from flygym_amd.vision import EyeRenderer, Scene

parser = argparse.ArgumentParser()
parser.add_argument("--seconds", type=float, default=3.0)
parser.add_argument("--flies", type=int, default=64)
parser.add_argument("--orbit", type=float, default=20.0, help="degrees per second the target moves round its fly (anticlockwise)")
parser.add_argument("--odor-gain", type=float, default=0.5, help="gain of the plume's odor (positive: attractive)")
args = parser.parse_args()

n = args.flies
STEPS = 20                                   # physics steps per control tick = one plume tick
DISTANCE, RADIUS = 8.0, 2.0                  # of the target from its fly, and the target's own (mm)
fly, world, _ = make_model()
sim = HIPSimulation(world, n_worlds=n, device=0)
sim.set_leg_adhesion_states(fly.name, np.ones((n, 6), dtype=np.float32))
sim.warmup()
tick_s = STEPS * sim.timestep
plume = OdorPlume(sim, fly.name, grid=(96, 160), cell_size=0.25, origin=(-8.0, -12.0), source=(10.0, 0.0, 1.0, 1.0), mean_wind=(-60.0, 0.0),
                  wind_tau=0.5, wind_sigma=60.0, diffusivity=1.0, tick_s=tick_s, seed=1)
eyes = EyeRenderer(sim, fly.name, scene=Scene(spheres=[(0.0, 0.0, -100.0, RADIUS)], sphere_rgb=[(0.0, 0.0, 0.0)]))
steer = SensorySteering(sim, fly.name, odor_gains=(args.odor_gain,))
# the targets: one per world, a tensor the renderer reads in place; world w's starts 40 degrees to the left or to the right
spheres = torch.zeros((n, 1, 4), dtype=torch.float32, device=sim.device)
spheres[:, 0, 2], spheres[:, 0, 3] = 1.3, RADIUS
eyes.set_spheres(spheres)
angle = torch.deg2rad(torch.where(torch.arange(n, device=sim.device) % 2 == 0, 40.0, -40.0))
omm = torch.zeros((n, 2, eyes.retina.num_ommatidia, 2), dtype=torch.float32, device=sim.device)
odor = torch.zeros((n, 1, 4), dtype=torch.float32, device=sim.device)


def move_targets():
    xy = sim.field("qpos")[:, :2]
    spheres[:, 0, 0] = xy[:, 0] + DISTANCE * torch.cos(angle)
    spheres[:, 0, 1] = xy[:, 1] + DISTANCE * torch.sin(angle)


with plume, TurningCPG(sim, fly.name) as cpg:
    plume.advance(int(round(0.4 / tick_s)))                 # let the plumes reach the flies before they start

    def tick():
        plume.advance()
        plume.get_odor_intensities(out=odor)
        eyes.render_into(omm)
        steer.update(omm=omm, odor=odor, out=cpg.drive)
        cpg.step(STEPS)

    move_targets()
    tick()                                                  # once eagerly: every kernel is loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tick()
    ticks = int(round(args.seconds / tick_s))
    in_view = torch.zeros(n, dtype=torch.int32, device=sim.device)
    smelled = torch.zeros(n, dtype=torch.bool, device=sim.device)
    for _ in range(ticks):
        angle += math.radians(args.orbit) * tick_s
        move_targets()
        graph.replay()
        in_view += (steer.features[:, :, 2] > 0.01).any(dim=1).to(torch.int32)
        smelled |= steer.bias != 0
    share = in_view.float() / ticks
    q = sim.field("qpos")
    yaw = torch.atan2(2 * (q[:, 3] * q[:, 6] + q[:, 4] * q[:, 5]), 1 - 2 * (q[:, 5] ** 2 + q[:, 6] ** 2))
    bearing = torch.rad2deg(torch.remainder(angle - yaw + math.pi, 2 * math.pi) - math.pi)
    print(f"{n} flies, {args.seconds:g} s ({ticks} replays of one captured tick): {int((share >= 0.9).sum())} kept the target in view for "
          f"at least 90 % of the ticks, {int((share >= 0.5).sum())} for at least half (mean share {float(share.mean()):.2f}); the target "
          f"ends {float(bearing.abs().mean()):.0f} degrees from the heading on average (it went round by {args.orbit * args.seconds:.0f}); "
          f"{int(smelled.sum())} flies smelled the plume; contact overflows {sim.overflow_steps()}")
