"""See motion with a retinotopic network: two groups of flies walk over the high-contrast checker ground of ``hold_a_course.py``
with the same base drive.  The open-loop gait curves; the first group is steered by the drive of a
``RetinotopicNetwork`` running ``sensors.motion_pathway()`` — 15 cell types per eye, its directional cells pooled into a rotation
signal — the second group's network runs too but steers nothing (``delta=0``).  Everything stays on the GPU: one control tick is
``eyes.render_into`` -> ``update`` of both networks (two launches each) -> two slice copies into ``cpg.drive`` -> ``cpg.step(20)``,
captured once as a graph and replayed.  Prints the yaw drift of each group and the pooled directional responses."""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
from flygym_amd import HIPSimulation, make_model
from flygym_amd.controllers import TurningCPG
from flygym_amd.sensors import RetinotopicNetwork, motion_pathway
from flygym_amd.vision import EyeRenderer, Scene

parser = argparse.ArgumentParser()
parser.add_argument("--seconds", type=float, default=1.0)
parser.add_argument("--flies", type=int, default=32, help="per group")
parser.add_argument("--checker", type=float, default=2.0, help="side of a ground square, mm")
parser.add_argument("--gain", type=float, default=None, help="steering gain (default: the class's)")
parser.add_argument("--substeps", type=int, default=2)
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
gain = {} if args.gain is None else dict(gain=args.gain)
network = motion_pathway()


def yaw():
    q = sim.field("qpos")
    return torch.atan2(2 * (q[:, 3] * q[:, 6] + q[:, 4] * q[:, 5]), 1 - 2 * (q[:, 5] ** 2 + q[:, 6] ** 2))


with TurningCPG(sim, fly.name) as cpg, RetinotopicNetwork(sim, fly.name, network, dt=tick_s, substeps=args.substeps, **gain) as seeing, \
        RetinotopicNetwork(sim, fly.name, network, dt=tick_s, substeps=args.substeps, delta=0.0) as blind:
    def tick():
        eyes.render_into(omm)
        seeing.update(omm)
        blind.update(omm)
        cpg.drive[:g] = seeing.drive[:g]
        cpg.drive[g:] = blind.drive[g:]
        cpg.step(STEPS)

    start, where = yaw().clone(), sim.field("qpos")[:, :2].clone()
    tick()                                                  # once eagerly: every kernel is loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tick()
    ticks = int(round(args.seconds / tick_s))
    signal = torch.zeros(n, device=sim.device)
    pooled = torch.zeros((n, 2, seeing.n_types), device=sim.device)
    for _ in range(ticks):
        graph.replay()
        signal += blind.signal
        pooled += blind.pooled
    turn = torch.rad2deg(torch.remainder(yaw() - start + torch.pi, 2 * torch.pi) - torch.pi)
    path = (sim.field("qpos")[:, :2] - where).norm(dim=1)
    print(f"2 x {g} flies, {args.seconds:g} s over a {args.checker:g} mm checker, {seeing.n_types} cell types, {args.substeps} sub-steps, "
          f"{ticks} replays of one captured tick; contact overflows {sim.overflow_steps()}")
    for name, s in (("steered  ", slice(0, g)), ("unsteered", slice(g, n))):
        print(f"  {name}: yaw drift mean {float(turn[s].mean()):+.1f} deg (spread {float(turn[s].std()):.1f}, mean |drift| "
              f"{float(turn[s].abs().mean()):.1f}), {float(path[s].mean()):.2f} mm from the start, mean signal "
              f"{float(signal[s].mean()) / ticks:+.2e}")
        mean = (pooled[s].mean(dim=0) / ticks).cpu().numpy()
        for c, kind in enumerate(seeing.type_names):
            if kind.startswith("T"):
                print(f"    {kind:7s} left {mean[0, c]:.4f}  right {mean[1, c]:.4f}")
