"""Hold a course with the optomotor reflex: two groups of flies walk over a high-contrast checker ground with the same drive.  The
open-loop gait curves; the first group's motion detectors (``MotionDetectors``) see the panorama turn and slow
the side it drifts towards, the second group's are switched off (``delta=0``).  Everything stays on the GPU: one control tick is
``eyes.render_into`` -> ``update`` of both detector sets (one launch each) -> two slice copies into ``cpg.drive`` -> ``cpg.step(20)``,
captured once as a graph and replayed.  Prints the yaw drift of each group."""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
from flygym_amd import HIPSimulation, make_model
from flygym_amd.controllers import TurningCPG
from flygym_amd.sensors import MotionDetectors
from flygym_amd.vision import EyeRenderer, Scene

parser = argparse.ArgumentParser()
parser.add_argument("--seconds", type=float, default=1.0)
parser.add_argument("--flies", type=int, default=32, help="per group")
parser.add_argument("--checker", type=float, default=2.0, help="side of a ground square, mm")
parser.add_argument("--gain", type=float, default=None, help="optomotor gain (default: the class's)")
parser.add_argument("--right", type=float, default=1.0, help="base drive of the right side (below 1: an imposed right turn)")
args = parser.parse_args()

g, n = args.flies, 2 * args.flies
STEPS = 20                                   # physics steps per control tick
fly, world, _ = make_model()
sim = HIPSimulation(world, n_worlds=n, device=0)
sim.set_leg_adhesion_states(fly.name, np.ones((n, 6), dtype=np.float32))
sim.warmup()
tick_s = STEPS * sim.timestep
eyes = EyeRenderer(sim, fly.name, scene=Scene(checker_size=args.checker, ground_rgb=((0, 0, 0), (1, 1, 1))))
omm = torch.zeros((n, 2, eyes.retina.num_ommatidia, 2), dtype=torch.float32, device=sim.device)
base = torch.tensor([[1.0, args.right]] * n, dtype=torch.float32, device=sim.device)
gain = {} if args.gain is None else dict(gain=args.gain)


def yaw():
    q = sim.field("qpos")
    return torch.atan2(2 * (q[:, 3] * q[:, 6] + q[:, 4] * q[:, 5]), 1 - 2 * (q[:, 5] ** 2 + q[:, 6] ** 2))


with TurningCPG(sim, fly.name) as cpg, MotionDetectors(sim, fly.name, dt=tick_s, **gain) as reflex, \
        MotionDetectors(sim, fly.name, dt=tick_s, delta=0.0) as off:
    def tick():
        eyes.render_into(omm)
        reflex.update(omm, base=base)
        off.update(omm, base=base)
        cpg.drive[:g] = reflex.drive[:g]
        cpg.drive[g:] = off.drive[g:]
        cpg.step(STEPS)

    start, where = yaw().clone(), sim.field("qpos")[:, :2].clone()
    tick()                                                  # once eagerly: every kernel is loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tick()
    ticks = int(round(args.seconds / tick_s))
    rotation = torch.zeros(n, device=sim.device)
    for _ in range(ticks):
        graph.replay()
        rotation += off.rotation
    turn = torch.rad2deg(torch.remainder(yaw() - start + torch.pi, 2 * torch.pi) - torch.pi)
    path = (sim.field("qpos")[:, :2] - where).norm(dim=1)
    print(f"2 x {g} flies, {args.seconds:g} s over a {args.checker:g} mm checker, base drive (1, {args.right:g}), "
          f"{ticks} replays of one captured tick; contact overflows {sim.overflow_steps()}")
    for name, s in (("reflex on ", slice(0, g)), ("reflex off", slice(g, n))):
        print(f"  {name}: yaw drift mean {float(turn[s].mean()):+.1f} deg (spread {float(turn[s].std()):.1f}, mean |drift| "
              f"{float(turn[s].abs().mean()):.1f}), {float(path[s].mean()):.2f} mm from the start, mean rotation signal "
              f"{float(rotation[s].mean()) / ticks:+.2e}")
