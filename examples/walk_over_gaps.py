"""Walk over the gapped terrain with and without the sensory rules: two batches of flies on ``GappedTerrainWorld``, one driven by
``TurningCPG`` and one by ``HybridTurningCPG`` (the same CPG plus the retraction and stumbling rules, decided on the GPU from the
batch's pose and contact sensors once per 20-step tick).  Prints the distance travelled and how often each rule fired.
``--terrain blocks`` / ``mixed`` walks the other rough terrains."""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
import flygym_amd.compose as C
from flygym_amd import HIPSimulation, make_model
from flygym_amd.controllers import HybridTurningCPG, TurningCPG
from flygym_amd.utils.math import Rotation3D

parser = argparse.ArgumentParser()
parser.add_argument("--seconds", type=float, default=1.0)
parser.add_argument("--worlds", type=int, default=16, help="flies per group")
parser.add_argument("--terrain", choices=("gapped", "blocks", "mixed"), default="gapped")
args = parser.parse_args()

WORLDS = {"gapped": C.GappedTerrainWorld, "blocks": C.BlocksTerrainWorld, "mixed": C.MixedTerrainWorld}
n, ticks = args.worlds, int(round(args.seconds / (20 * 1e-4)))
for cls in (TurningCPG, HybridTurningCPG):
    fly = make_model()[0]
    world = WORLDS[args.terrain]()
    world.add_fly(fly, (0, 0, 0.8), Rotation3D("quat", (1, 0, 0, 0)))
    sim = HIPSimulation(world, n_worlds=n, device=0)
    sim.set_leg_adhesion_states(fly.name, np.ones((n, 6), dtype=np.float32))
    sim.warmup()
    start = sim.field("qpos")[:, :2].clone()
    fired = torch.zeros(2, dtype=torch.int64, device=sim.device)
    with cls(sim, fly.name) as cpg:
        for _ in range(ticks):
            cpg.step(20)
            if cls is HybridTurningCPG:
                fired += torch.stack([((cpg.rule_flags & 1) != 0).any(dim=1).sum(), ((cpg.rule_flags & 2) != 0).any(dim=1).sum()])
    moved = (sim.field("qpos")[:, :2] - start).cpu().numpy()
    finite = bool(torch.isfinite(sim.field("qpos")).all())
    line = (f"{args.terrain}, {cls.__name__}, {n} flies, {ticks} ticks of 20 steps: x travelled {moved[:, 0].mean():+.2f} mm "
            f"(min {moved[:, 0].min():+.2f}, max {moved[:, 0].max():+.2f}), |y| {np.abs(moved[:, 1]).mean():.2f} mm, finite {finite}, "
            f"contact overflow steps {sim.overflow_steps()}")
    if cls is HybridTurningCPG:
        f = fired.cpu().numpy()
        line += f"; world-ticks with a retraction {f[0]} ({f[0] / (n * ticks):.1%}), with a stumble {f[1]} ({f[1] / (n * ticks):.1%})"
    print(line, flush=True)
