"""Navigate an intermittent odor plume: the arena and the plumes of ``track_a_plume.py`` (256 flies, each in its own plume that a
noisy wind blows from a source 10 mm ahead), steered by ``PlumeNavigator`` — a walk / stop / turn state machine per fly that is
driven by odor onsets and turns upwind the more often the more onsets it has met.  The whole control tick is ONE captured graph:
``plume.advance()``, the antennal readings into a fixed buffer, ``nav.update(buf, plume.wind, out=cpg.drive)`` and ``cpg.step(20)``;
the navigator's noise counter lives on the device, so every replay draws fresh noise.  Prints how many flies reached the source and
how many left the arena, and the same counts for the antennal-asymmetry rule of ``track_a_plume.py`` run on the same plumes."""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
from flygym_amd import HIPSimulation, make_model
from flygym_amd.controllers import PlumeNavigator, TurningCPG
from flygym_amd.sensors import OdorPlume

parser = argparse.ArgumentParser()
parser.add_argument("--seconds", type=float, default=2.0)
parser.add_argument("--flies", type=int, default=256)
parser.add_argument("--threshold", type=float, default=0.02, help="antennal sum above which the navigator counts odor as present")
parser.add_argument("--p-up", type=float, nargs=2, default=(0.5, 0.15), metavar=("BASE", "GAIN"), help="probability that a turn goes upwind: "
                    "BASE + GAIN x encounter frequency")
parser.add_argument("--turn-duration", type=float, default=0.25, help="seconds a turn lasts")
parser.add_argument("--turn-drive", type=float, nargs=2, default=(-0.4, 1.2), metavar=("INNER", "OUTER"), help="the CPG's drive during a turn")
parser.add_argument("--gain", type=float, default=2.0, help="the asymmetry rule's drive change per unit of (L - R) / (L + R)")
parser.add_argument("--seed", type=int, default=1)
args = parser.parse_args()

n = args.flies
STEPS = 20                                   # physics steps per control tick = one plume tick
SOURCE = (10.0, 0.0, 1.0, 1.0)               # x, y, radius (mm), peak
fly, world, _ = make_model()
sim = HIPSimulation(world, n_worlds=n, device=0)
sim.set_leg_adhesion_states(fly.name, np.ones((n, 6), dtype=np.float32))
sim.warmup()
tick_s = STEPS * sim.timestep
n_ticks = int(round(args.seconds / tick_s))
goal = torch.tensor(SOURCE[:2], device=sim.device)


def run(name, plume, tick):
    """``n_ticks`` control ticks after a :func:`start`; ``tick()`` is one whole control tick."""
    left_arena = torch.zeros(n, dtype=torch.bool, device=sim.device)
    nearest = torch.full((n,), float("inf"), device=sim.device)
    for _ in range(n_ticks):
        tick()
        left_arena |= plume.out_of_bounds.bool()
        nearest = torch.minimum(nearest, (sim.field("qpos")[:, :2] - goal).norm(dim=1))
    reached = nearest < SOURCE[2] + 1.0
    walked = sim.field("qpos")[:, 0]
    print(f"{name}: {n} flies, {args.seconds:g} s: {int(reached.sum())} reached the source, {int((left_arena & ~reached).sum())} left the "
          f"arena; walked {float(walked.mean()):.1f} mm along x on average (max {float(walked.max()):.1f}), nearest approach "
          f"{float(nearest.min()):.1f} mm")
    return int(reached.sum()), int((left_arena & ~reached).sum())


def start(plume, cpg):
    sim.reset()
    cpg.reset()
    plume.reset()
    plume.advance(int(round(0.4 / plume.tick_s)))            # let the plumes reach the flies before they start


# the arena of track_a_plume.py: 24 mm x 40 mm of quarter-millimetre cells, a meandering 60 mm/s wind from the source to the flies
plume = OdorPlume(sim, fly.name, grid=(96, 160), cell_size=0.25, origin=(-8.0, -12.0), source=SOURCE, mean_wind=(-60.0, 0.0),
                  wind_tau=0.5, wind_sigma=60.0, diffusivity=1.0, tick_s=tick_s, seed=args.seed)
buf = torch.zeros((n, 1, 4), dtype=torch.float32, device=sim.device)
with plume, TurningCPG(sim, fly.name) as cpg, PlumeNavigator(
        sim, fly.name, tick_s=tick_s, threshold=args.threshold, seed=args.seed, p_up=tuple(args.p_up), turn_duration=args.turn_duration,
        turn_drive=tuple(args.turn_drive)) as nav:
    def navigator_tick():
        plume.advance()
        plume.get_odor_intensities(out=buf)
        nav.update(buf, plume.wind, out=cpg.drive)
        cpg.step(STEPS)

    def asymmetry_tick():
        plume.advance()
        odor = plume.get_odor_intensities(out=buf)[:, 0]              # (n, 4): palps left / right, antennae left / right
        left, right = odor[:, 2], odor[:, 3]
        turn = args.gain * (left - right) / (left + right + 1e-6)     # > 0: more odor on the left, slow the left legs down
        cpg.drive.copy_(torch.stack([1.0 - turn, 1.0 + turn], dim=1).clamp(0.2, 1.2))
        cpg.step(STEPS)

    start(plume, cpg)
    navigator_tick()                                         # one eager tick: every kernel of the chain has run before the capture
    start(plume, cpg)
    nav.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        navigator_tick()
    counts = {"navigator": run("PlumeNavigator (one graph per tick)", plume, graph.replay)}
    states = torch.bincount(nav.state.long(), minlength=4).tolist()
    print(f"  encounters per fly {float(nav.encounters.float().mean()):.1f} (max {int(nav.encounters.max())}); now walking / stopped / "
          f"turning left / right: {states}")
    start(plume, cpg)
    counts["asymmetry"] = run("antennal asymmetry (track_a_plume.py's rule)", plume, asymmetry_tick)
    print(f"reached the source: navigator {counts['navigator'][0]}, asymmetry rule {counts['asymmetry'][0]} of {n}; left the arena: "
          f"navigator {counts['navigator'][1]}, asymmetry rule {counts['asymmetry'][1]}")
