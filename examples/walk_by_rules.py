"""Walk by Cruse's rules: 256 flies on flat ground for 1 s under ``RuleBasedController`` (default graph and weights, adhesion on), one
captured graph per 20-step control tick, and beside them 256 flies under ``TurningCPG``.  No gait is programmed for the first group:
each leg starts a step when the rules, scored from the other legs' step counters, say so.

Prints, per controller, the median forward distance of the thorax, the number of flies whose thorax stayed above half its starting
height, and how many legs were in swing per physics step (the adhesion columns of the rows written)."""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
from flygym_amd import HIPSimulation, make_model
from flygym_amd.controllers import RuleBasedController, TurningCPG

parser = argparse.ArgumentParser()
parser.add_argument("--worlds", type=int, default=256)
parser.add_argument("--seconds", type=float, default=1.0)
parser.add_argument("--seed", type=int, default=0)
args = parser.parse_args()

STEPS, ADHESION = 20, (20.0, 1.0)
n = args.worlds


def walk(name, make):
    fly, world, _ = make_model()
    sim = HIPSimulation(world, n_worlds=n, device=0)
    sim.set_leg_adhesion_states(fly.name, np.ones((n, 6), dtype=np.float32))
    sim.warmup()
    root = [s.name for s in fly.get_bodysegs_order()].index(fly.root_segment.name)
    with make(sim, fly) as ctl:
        ctl.step(STEPS)                                    # every kernel of the tick has run before the capture
        thorax = sim.field("seg_xpos").view(n, sim.model.nseg, 3)[:, root]   # a view: the thorax in the world, as it stands
        start = thorax.clone()
        lowest = start[:, 2].clone()
        swinging = torch.zeros(7, dtype=torch.int64, device=sim.device)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ctl.step(STEPS)
        for _ in range(int(round(args.seconds / (STEPS * sim.timestep)))):
            graph.replay()
            lowest = torch.minimum(lowest, thorax[:, 2])
            lifted = (ctl.table[:, :STEPS, -6:] == ADHESION[1]).sum(dim=2)
            swinging += torch.bincount(lifted.flatten(), minlength=7)
        torch.cuda.synchronize()
        forward = (thorax[:, 0] - start[:, 0]).cpu().numpy()
        upright = int((lowest > 0.5 * start[:, 2]).sum())
        finite = bool(torch.isfinite(sim.field("qpos")).all())
    share = (swinging.double() / swinging.sum()).cpu().numpy()
    print(f"{name}: {n} flies, {args.seconds:g} s: median forward distance {np.median(forward):+.2f} mm (min {forward.min():+.2f}, max "
          f"{forward.max():+.2f}); {upright} of {n} kept the thorax above half its starting height; state finite: {finite}")
    print("  legs in swing per step, share of steps with 0..6: " + " ".join(f"{s:.3f}" for s in share))


walk("RuleBasedController", lambda sim, fly: RuleBasedController(sim, fly.name, adhesion=ADHESION, seed=args.seed))
walk("TurningCPG", lambda sim, fly: TurningCPG(sim, fly.name, adhesion=ADHESION))
