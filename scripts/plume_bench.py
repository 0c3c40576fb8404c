"""Time ``OdorPlume.advance`` on the GPU: 4096 plumes of 128 x 256 cells (1 GiB of state across both buffers, four times the
Infinity Cache), against the traffic model of one read and one write of the grid per tick, and against a 50-step control tick of
the same 4096 flies walking on the closed-loop tripod CPG (``TurningCPG.step``).

Device events around windows of --ticks ticks, after a warm-up of the same shape; --repeats windows, median and spread reported.
A tick is two launches (the grid kernel, then the one-lane-per-plume wind kernel): the time is that of the pair.  Results go to
stdout and, as JSON, to --out (recorded by hand in profiles/plume_summary.md).  Needs an MI355X: no fallback."""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
from flygym_amd import HIPSimulation, make_model
from flygym_amd.controllers import TurningCPG
from flygym_amd.sensors import OdorPlume

parser = argparse.ArgumentParser()
parser.add_argument("--plumes", type=int, default=4096)
parser.add_argument("--grid", type=int, nargs=2, default=(128, 256))
parser.add_argument("--ticks", type=int, default=200)
parser.add_argument("--repeats", type=int, default=7)
parser.add_argument("--control-steps", type=int, default=50)
parser.add_argument("--out", type=Path, default=None)
args = parser.parse_args()
if not torch.cuda.is_available():
    sys.exit("plume_bench.py measures on the GPU and found none")

n, (H, W) = args.plumes, args.grid
fly, world, _ = make_model()
sim = HIPSimulation(world, n_worlds=n, device=0)
sim.set_leg_adhesion_states(fly.name, np.ones((n, 6), dtype=np.float32))
sim.warmup()


def timed(fn, repeats):
    """Milliseconds of each of `repeats` calls of fn, by device events on the simulation's stream."""
    out = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        out.append(t0.elapsed_time(t1))
    return out


# the control tick the plume runs beside: the closed-loop CPG's launch plus control_steps physics steps of every fly
steps = args.control_steps
with TurningCPG(sim, fly.name) as cpg:
    for _ in range(40):                            # a gait cycle and more: the flies walk
        cpg.step(steps)
    control_ms = timed(lambda: cpg.step(steps), 40)

result = dict(plumes=n, grid=[H, W], ticks_per_window=args.ticks, repeats=args.repeats, control_steps=steps,
              state_bytes=2 * n * H * W * 4, model_bytes_per_tick=2 * n * H * W * 4,
              control_tick_ms=dict(median=statistics.median(control_ms), min=min(control_ms), max=max(control_ms)), variants={})
jj, ii = np.mgrid[0:H, 0:W]
eddies = 30.0 * np.stack([np.sin(2 * np.pi * jj / H) * np.cos(np.pi * ii / W), np.cos(2 * np.pi * ii / W)], axis=-1).astype(np.float32)
for name, kw in (("wind only", dict(eddies=None)), ("wind + eddies", dict(eddies=eddies, eddy_gain=1.0))):
    with OdorPlume(sim, fly.name, grid=(H, W), cell_size=0.25, origin=(0.0, 0.0), source=(8.0, H * 0.125, 1.0, 1.0), mean_wind=(40.0, 0.0),
                   wind_tau=0.5, wind_sigma=30.0, diffusivity=1.0, tick_s=0.005, seed=3, **kw) as plume:
        plume.advance(args.ticks)                  # warm-up of the timed shape; the plumes fill
        ms = [t / args.ticks for t in timed(lambda: plume.advance(args.ticks), args.repeats)]
        med = statistics.median(ms)
        filled = float((plume.concentration() > 1e-3).float().mean())
        result["variants"][name] = dict(ms_per_tick=dict(median=med, min=min(ms), max=max(ms)),
                                        model_tb_per_s=result["model_bytes_per_tick"] / (med * 1e-3) / 1e12,
                                        share_of_control_tick=med / result["control_tick_ms"]["median"], cells_above_1e3=filled)
        print(f"{name:14s}: {med * 1e3:8.1f} us per tick (min {min(ms) * 1e3:.1f}, max {max(ms) * 1e3:.1f}) = "
              f"{result['variants'][name]['model_tb_per_s']:.2f} TB/s of the model's 2 x {n * H * W * 4 / 2**20:.0f} MiB; "
              f"{100 * result['variants'][name]['share_of_control_tick']:.2f} % of a {steps}-step control tick "
              f"({result['control_tick_ms']['median']:.3f} ms); {100 * filled:.1f} % of the cells above 1e-3")
print(json.dumps(result))
if args.out is not None:
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(result, indent=1) + "\n")
