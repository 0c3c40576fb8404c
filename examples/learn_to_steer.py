"""Learn to steer towards a goal, with no RL library: a cross-entropy search over linear policies from the twelve body-level
observation floats of ``WalkingTask`` (gravity direction, linear and angular velocity, goal direction — all in the body frame — and
height) to the two drives of a ``TurningCPG``.  256 flies walk one episode per generation, each towards its own goal on a ring
around the spawn point; four flies with goals a quarter turn apart share a candidate policy, whose score is their mean return, so
that a candidate is not ranked by where its goal happened to lie.  The whole control tick — the CPG, 20 physics steps, the task's
update and the resets of the worlds that ended — is ONE captured graph (``TaskEnv(capture=True)``), the policies are one
``torch.bmm`` per tick, and nothing in the loop waits for the device: no ``.any()``, no ``.item()``.  After a generation the best
fifth of the candidates refits the search distribution.  Prints per generation the mean return, how many flies reached their goal,
why the episodes ended and how long the generation took.  Nothing about the outcome is promised: the numbers are what a run prints."""
import argparse
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
from flygym_amd import HIPSimulation, TaskEnv, WalkingTask, make_model
from flygym_amd.controllers import TurningCPG
from flygym_amd.tasks import REASONS

parser = argparse.ArgumentParser()
parser.add_argument("--flies", type=int, default=256)
parser.add_argument("--generations", type=int, default=6)
parser.add_argument("--seconds", type=float, default=1.0, help="length of an episode")
parser.add_argument("--ring", type=float, default=3.0, help="radius (mm) of the ring of goals around the spawn point")
parser.add_argument("--sigma", type=float, default=0.3, help="initial standard deviation of the policy weights")
parser.add_argument("--seed", type=int, default=0)
args = parser.parse_args()

n, STEPS, PER = args.flies, 20, 4                     # PER worlds, goals a quarter turn apart, per candidate policy
if n % PER:
    sys.exit(f"--flies must be a multiple of {PER}")
m = n // PER
fly, world, _ = make_model()
sim = HIPSimulation(world, n_worlds=n, device=0)
sim.set_leg_adhesion_states(fly.name, np.ones((n, 6), dtype=np.float32))
dev = sim.device
ticks = int(round(args.seconds / (STEPS * sim.timestep)))
cpg = TurningCPG(sim, fly.name, table_steps=32)
task = WalkingTask(sim, fly.name, max_ticks=ticks, goal_radius=0.5, alive=0.0, w_progress=1.0, w_power=0.0, w_tilt=0.1, bonus_goal=5.0,
                   penalty_fail=1.0)
env = TaskEnv(sim, cpg, task, steps_per_tick=STEPS, capture=True)
spawn = sim.field("qpos")[:, :2].clone()
w = torch.arange(n, device=dev)
angle = 2 * np.pi * ((w % PER) / PER + (w // PER) / n)  # candidate c's goals: c / n of a turn past 0, 1/4, 1/2, 3/4
ring = torch.stack([torch.cos(angle), torch.sin(angle)], dim=1)
task.set_goal(spawn + args.ring * ring)
task.set_course(ring)                                   # progress counts along the spawn-to-goal direction

# a policy: drive = clip(W [obs / scale; 1]); the search starts at "walk straight on" (the bias row alone, drive (1, 1))
scale = torch.tensor([1, 1, 1, 20, 20, 20, 20, 20, 20, 3, 3, 1], dtype=torch.float32, device=dev)
gen = torch.Generator(device=dev).manual_seed(args.seed)
mean = torch.zeros((2, 13), device=dev)
mean[:, 12] = 1.0
std = torch.full((2, 13), args.sigma, device=dev)
x = torch.ones((n, 13, 1), device=dev)
print(f"{n} flies = {m} candidate policies x {PER} goals, {args.generations} generations of one {args.seconds:g} s episode ({ticks} ticks of "
      f"{STEPS} steps), goals on a ring of {args.ring:g} mm; one captured graph per tick")
for g in range(args.generations):
    t0 = time.perf_counter()
    cand = mean + std * torch.randn((m, 2, 13), generator=gen, device=dev)
    cand[0] = mean                                      # (the distribution's mean itself is a candidate)
    W = cand.repeat_interleave(PER, dim=0)
    obs = env.reset()
    ret = torch.zeros(n, device=dev)
    why = torch.zeros(n, dtype=torch.int32, device=dev)
    ended = torch.zeros(n, dtype=torch.bool, device=dev)
    for _ in range(ticks - 1):                          # (the reset's own update was the first tick)
        x[:, :12, 0] = obs[:, :12] / scale
        obs, reward, terminated, truncated, info = env.step(torch.bmm(W, x)[:, :, 0].clamp(-0.5, 1.5))
        first = ~ended & (info["episodes"] > 0)         # a world's first episode of this generation just ended
        ret = torch.where(first, info["last_return"], ret)
        why = torch.where(first, task.last_reason, why)
        ended |= first
    score = ret.view(m, PER).mean(dim=1)
    elite = score.topk(max(m // 5, 2)).indices
    mean, std = cand[elite].mean(dim=0), cand[elite].std(dim=0) + 0.02
    why_host, ret_host, score_host = why.cpu().numpy(), ret.cpu().numpy(), score.cpu().numpy()      # the generation's one synchronisation
    hist = {name: int(((why_host & bit) != 0).sum()) for name, bit in REASONS.items() if ((why_host & bit) != 0).any()}
    hist["time_limit"] = int((why_host == 0).sum())
    print(f"generation {g}: mean return {ret_host.mean():7.3f} (best candidate {score_host.max():.3f}, elite mean {score_host[elite.cpu().numpy()].mean():.3f}, "
          f"the distribution's mean {score_host[0]:.3f}), "
          f"{hist.get('goal', 0)} of {n} reached their goal, episodes ended by {hist}; {time.perf_counter() - t0:.2f} s")
task.close()
cpg.close()
