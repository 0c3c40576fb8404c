"""Path integration: 256 flies walk under the closed-loop tripod CPG with piecewise-constant random drives while a
``PathIntegrator`` estimates each one's heading and position from its legs' stance strides alone (the form of flygym 1.x's
path-integration task).  The first 2 s are recorded on one half of the worlds to calibrate the 14 shared coefficients
(``PathIntegrator.calibrate``); then the estimates start from the true pose and the other half is scored over 3 s, every control
tick — ``cpg.step(20)`` + ``integrator.update()`` — being one captured graph that is replayed.  Prints the seed, the fits' R^2, and
the median and 90th percentile of |estimated - true position| / path length and of the heading error at the end."""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
from flygym_amd import HIPSimulation, make_model
from flygym_amd.controllers import TurningCPG
from flygym_amd.sensors import PathIntegrator

parser = argparse.ArgumentParser()
parser.add_argument("--worlds", type=int, default=256)
parser.add_argument("--calibrate-s", type=float, default=2.0)
parser.add_argument("--test-s", type=float, default=3.0)
parser.add_argument("--window-s", type=float, default=0.32, help="the stride window (flygym 1.x used 0.32 s and 0.64 s)")
parser.add_argument("--drive-s", type=float, default=0.25, help="how long a random drive is held")
parser.add_argument("--seed", type=int, default=0)
args = parser.parse_args()

STEPS = 20
n, half = args.worlds, args.worlds // 2
fly, world, _ = make_model()
sim = HIPSimulation(world, n_worlds=n, device=0)
sim.set_leg_adhesion_states(fly.name, np.ones((n, 6), dtype=np.float32))
sim.warmup()
tick_s = STEPS * sim.timestep
window = max(1, int(round(args.window_s / tick_s)))
hold = max(1, int(round(args.drive_s / tick_s)))
rng = np.random.default_rng(args.seed)
print(f"seed {args.seed}: {n} flies, control tick {tick_s * 1e3:.1f} ms, window {window} ticks, a new random drive every {hold} ticks")


def wrap(a):
    return torch.remainder(a + np.pi, 2 * np.pi) - np.pi


with TurningCPG(sim, fly.name, table_steps=STEPS) as cpg, PathIntegrator(sim, fly.name, window=window) as odo:
    staged = torch.ones((n, 2), dtype=torch.float32, device=sim.device)

    def new_drive():
        staged.copy_(torch.as_tensor(rng.uniform(0.4, 1.2, (n, 2)).astype(np.float32)))
        cpg.drive.copy_(staged)

    # ---- 2 s recorded on the first half of the worlds
    T = int(round(args.calibrate_s / tick_s))
    strides = torch.zeros((T, half, 6), dtype=torch.float64, device=sim.device)
    poses = torch.zeros((T, half, 3), dtype=torch.float64, device=sim.device)
    for k in range(T):
        if k % hold == 0:
            new_drive()
        cpg.step(STEPS)
        odo.update()
        strides[k] = odo.window_strides[:half]
        poses[k] = odo.true_pose()[:half]
    coef, r2_heading, r2_disp = PathIntegrator.calibrate(strides.cpu().numpy(), poses.cpu().numpy(), window)
    odo.set_coefficients(coef[:6], coef[6:12], coef[12], coef[13])
    print(f"calibrated on worlds 0..{half - 1} over {T} ticks: R^2 heading {r2_heading:.4f}, displacement {r2_disp:.4f}")
    print("  heading_coef", np.array2string(coef[:6], precision=4), "bias", f"{coef[12]:+.5f}")
    print("  disp_coef   ", np.array2string(coef[6:12], precision=4), "bias", f"{coef[13]:+.5f}")

    # ---- 3 s scored on the other half: the estimate starts from the truth, every tick is one replay of one graph
    start = odo.true_pose().clone()
    odo.position.copy_(start[:, :2])
    odo.heading.copy_(start[:, 2])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cpg.step(STEPS)
        odo.update()
    # (the capture ran nothing: the first replay is the first tick)
    last = start[:, :2].clone()
    path = torch.zeros(n, dtype=torch.float64, device=sim.device)
    for k in range(int(round(args.test_s / tick_s))):
        if k % hold == 0:
            new_drive()
        graph.replay()
        now = odo.true_pose()[:, :2]
        path += torch.linalg.norm(now - last, dim=1)
        last = now.clone()
    truth = odo.true_pose()
    score = slice(half, n)
    rel = (torch.linalg.norm(odo.position - truth[:, :2], dim=1) / path)[score].cpu().numpy()
    head = torch.rad2deg(wrap(odo.heading - truth[:, 2]).abs())[score].cpu().numpy()
    turned = torch.rad2deg(wrap(truth[:, 2] - start[:, 2]).abs())[score].cpu().numpy()
    home = torch.linalg.norm(odo.home, dim=1)[score].cpu().numpy()
    print(f"scored on worlds {half}..{n - 1} over {args.test_s:g} s: path length median {np.median(path[score].cpu().numpy()):.2f} mm, "
          f"|heading change| median {np.median(turned):.1f} deg")
    print(f"  |estimated - true position| / path length: median {np.median(rel):.4f}, 90th percentile {np.percentile(rel, 90):.4f}")
    print(f"  heading error at the end: median {np.median(head):.2f} deg, 90th percentile {np.percentile(head, 90):.2f} deg")
    print(f"  distance home by the estimate: median {np.median(home):.2f} mm; all finite: {bool(torch.isfinite(odo.position).all())}")
