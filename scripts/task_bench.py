"""Time ``WalkingTask.update`` on the GPU: 4096 worlds with the default 42 actuators and 42 observed dofs, against the same rule
written with torch operations on the same data (``TorchRule`` below: kept here, not in the package), against the 20-step control
tick it belongs to, and one whole ``TaskEnv.step`` eager against captured.

The two flavours alternate in the same process after a warm-up; each is timed by device events over windows of --calls calls until
at least --seconds have been measured: calls issued from Python back to back, so a figure near 10 us is as much the host's issue
rate as the kernel.  The kernel is therefore also timed as --calls updates captured into one graph and replayed.  Before the timing
both flavours follow --ticks ticks of a real walk and what they decided is compared.  Results go to stdout and, as JSON, to --out
(recorded by hand in profiles/task_summary.md).  Needs an MI355X: no fallback."""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
from flygym_amd import HIPSimulation, make_model
from flygym_amd.controllers import TurningCPG, _leg_contact_flags
from flygym_amd.tasks import TaskEnv, WalkingTask

parser = argparse.ArgumentParser()
parser.add_argument("--worlds", type=int, default=4096)
parser.add_argument("--ticks", type=int, default=100)
parser.add_argument("--calls", type=int, default=50)
parser.add_argument("--seconds", type=float, default=0.5)
parser.add_argument("--control-steps", type=int, default=20)
parser.add_argument("--out", type=Path, default=None)
args = parser.parse_args()
if not torch.cuda.is_available():
    sys.exit("task_bench.py measures on the GPU and found none")

n, steps = args.worlds, args.control_steps
fly, world, _ = make_model()
sim = HIPSimulation(world, n_worlds=n, device=0)
sim.set_leg_adhesion_states(fly.name, np.ones((n, 6), dtype=np.float32))
sim.warmup()
dev = sim.device
KW = dict(max_ticks=40, goal_radius=0.5, alive=0.01, w_progress=1.0, w_power=1e-4, w_tilt=0.1, bonus_goal=5.0, penalty_fail=1.0)
task = WalkingTask(sim, fly.name, **KW)
P = task._params
nseg = sim.model.nseg
ids = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int64), device=dev)
ACT, ACT_DOF, OBS_DOF = ids(task._act), ids(6 + task._act_dof), ids(7 + task._obs_dof)
THR2 = torch.as_tensor(task.thr2, device=dev)
MEAN, INV_STD = torch.as_tensor(task._mean, device=dev), torch.as_tensor(task._inv_std, device=dev)
ODD = 0x7F800000


def odd(a):
    return ((a.contiguous().view(torch.int32) & ODD) == ODD).reshape(n, -1).any(dim=1)


class TorchRule:
    """The update in torch operations on tensors of its own (float32 throughout, each operation rounded on its own as in the kernel)."""

    def __init__(self):
        z = lambda dtype, *shape: torch.zeros((n, *shape), dtype=dtype, device=dev)
        self.fresh = torch.ones(n, dtype=torch.bool, device=dev)
        self.prev_xy, self.course, self.goal = z(torch.float32, 2), task.course.clone(), task.goal.clone()
        self.tilt_count, self.airborne_count, self.ep_length = z(torch.int32), z(torch.int32), z(torch.int32)
        self.ep_return, self.last_return = z(torch.float32), z(torch.float32)
        self.last_length, self.last_reason, self.episodes, self.successes = (z(torch.int32) for _ in range(4))

    def update(self):
        pos = sim.field("seg_xpos").view(n, nseg, 3)[:, task.root_seg]
        quat = sim.field("seg_xquat").view(n, nseg, 4)[:, task.root_seg]
        qvel, qpos = sim.field("qvel"), sim.field("qpos")
        vel, force, qd, ang = qvel[:, :6], sim.field("actuator_force")[:, ACT], qvel[:, ACT_DOF], qpos[:, OBS_DOF]
        sens = sim.field("sensordata").view(n, 6, 16)[:, :, :4]
        x, y, z = pos.unbind(dim=1)
        qw, qx, qy, qz = quat.unbind(dim=1)
        vx, vy, vz, ox, oy, oz = vel.unbind(dim=1)
        bad = odd(pos) | odd(quat) | odd(vel) | odd(force) | odd(qd) | odd(sens) | odd(ang) | odd(self.course) | odd(self.goal)
        progress = torch.where(self.fresh, 0.0, (x - self.prev_xy[:, 0]) * self.course[:, 0] + (y - self.prev_xy[:, 1]) * self.course[:, 1])
        up_z = 1 - 2 * (qx * qx + qy * qy)
        tilt = torch.where(up_z < P.cos_max_tilt, self.tilt_count + 1, 0)
        flags = _leg_contact_flags(torch, sim.field("sensordata"), THR2)
        air = torch.where(flags.sum(dim=1) == 0, self.airborne_count + 1, 0)
        m = (force * qd).abs()
        c = torch.where(m > P.power_clip, P.power_clip, m)
        finite = ((force.contiguous().view(torch.int32) & ODD) != ODD) & ((qd.contiguous().view(torch.int32) & ODD) != ODD)
        power = torch.round(torch.where(finite, c * 1024.0, 0.0)).to(torch.int32).sum(dim=1, dtype=torch.int32).to(torch.float32) * (1 / 1024)
        length = self.ep_length + 1
        grace = length <= P.grace_ticks
        dx, dy = self.goal[:, 0] - x, self.goal[:, 1] - y
        reason = (torch.where(~grace & (tilt >= P.tilt_ticks), 2, 0) | torch.where(~grace & (air >= P.airborne_ticks), 4, 0)
                  | torch.where(~grace & ((z < P.z_min) | (z > P.z_max)), 8, 0)
                  | torch.where((x < P.arena[0]) | (x > P.arena[1]) | (y < P.arena[2]) | (y > P.arena[3]), 16, 0)
                  | torch.where(dx * dx + dy * dy < P.goal_radius2, 32, 0))
        reason = torch.where(bad, 1, reason).to(torch.int32)
        terminated = reason != 0
        truncated = ~terminated & (length >= P.max_ticks)
        done = terminated | truncated
        r = P.alive + P.w_progress * progress
        r = r - P.w_power * power
        r = r - P.w_tilt * (1 - up_z)
        r = torch.where((reason & 32) != 0, r + P.bonus_goal, r)
        r = torch.where((reason & ~32) != 0, r - P.penalty_fail, r)
        r = torch.where(bad, -P.penalty_fail, r)
        ret = self.ep_return + r
        r00, r01, r02 = 1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy)
        r10, r11, r12 = 2 * (qx * qy + qw * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qw * qx)
        r20, r21 = 2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx)
        body = torch.stack([-r20, -r21, -up_z, (r00 * vx + r10 * vy) + r20 * vz, (r01 * vx + r11 * vy) + r21 * vz,
                            (r02 * vx + r12 * vy) + up_z * vz, ox, oy, oz, r00 * dx + r10 * dy, r01 * dx + r11 * dy, z], dim=1)
        obs = torch.cat([body, flags, (ang - MEAN) * INV_STD], dim=1)
        self.obs = torch.where(bad[:, None], 0.0, obs + 0.0)
        self.reward, self.terminated, self.truncated, self.done, self.reason = r + 0.0, terminated, truncated, done, reason
        self.last_return = torch.where(done, ret, self.last_return)
        self.last_length = torch.where(done, length, self.last_length)
        self.last_reason = torch.where(done, reason, self.last_reason)
        self.episodes = self.episodes + done.to(torch.int32)
        self.successes = self.successes + (done & ((reason & 32) != 0)).to(torch.int32)
        self.ep_return = torch.where(done, 0.0, ret)
        self.ep_length = torch.where(done, 0, length)
        self.tilt_count, self.airborne_count = torch.where(done, 0, tilt), torch.where(done, 0, air)
        self.fresh = done
        self.prev_xy = torch.where(done[:, None], 0.0, torch.stack([x, y], dim=1))


def window(fn, calls):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for k in range(calls):
        fn(k)
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / calls          # microseconds per call


with TurningCPG(sim, fly.name, table_steps=32) as cpg:
    angle = torch.linspace(0, 2 * np.pi, n, device=dev)
    task.set_goal(torch.stack([3 * torch.cos(angle), 3 * torch.sin(angle)], dim=1))
    task.set_course(torch.stack([torch.cos(angle), torch.sin(angle)], dim=1))
    rule = TorchRule()
    mismatches = dict(reward=0, obs=0, done=0, reason=0, last_return=0, episodes=0)
    for _ in range(args.ticks):                        # both flavours follow the same walk; the kernel's mask resets it
        cpg.step(steps)
        rule.update()
        task.update()
        mismatches["reward"] += int((task.reward != rule.reward).sum())
        mismatches["obs"] += int((task.obs != rule.obs).any(dim=1).sum())
        mismatches["done"] += int((task.done != rule.done.to(torch.uint8)).sum())
        mismatches["reason"] += int((task.reason != rule.reason).sum())
        sim.reset_worlds(task.done)
        cpg.reset(task.done)
    mismatches["last_return"] = int((task.last_return != rule.last_return).sum())
    mismatches["episodes"] = int((task.episodes != rule.episodes).sum())
    agreement = dict(mismatches, world_ticks=n * args.ticks, stats=task.stats())
    ok = all(v == 0 for v in mismatches.values())

    variants = {"kernel": lambda k: task.update(), "torch": lambda k: rule.update()}
    for fn in variants.values():                       # warm-up of every timed shape
        window(fn, args.calls)
    times = {name: [] for name in variants}
    total = {name: 0.0 for name in variants}
    while min(total.values()) < args.seconds * 1e6:    # alternated: a window of each in turn
        for name, fn in variants.items():
            us = window(fn, args.calls)
            times[name].append(us)
            total[name] += us * args.calls

    # the same launch without the host between the calls: --calls updates captured as one graph (one chain), timed per replay
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(args.calls):
            task.update()
    for _ in range(3):
        window(lambda k: graph.replay(), 10)
    graph_us = statistics.median(window(lambda k: graph.replay(), 10) for _ in range(15)) / args.calls

    for _ in range(3):
        window(lambda k: cpg.step(steps), 10)
    bare_us = statistics.median(window(lambda k: cpg.step(steps), 10) for _ in range(7))

    # one whole TaskEnv.step, eager against captured, alternated on the same batch
    action = torch.ones((n, 2), dtype=torch.float32, device=dev)
    envs = {"eager": TaskEnv(sim, cpg, task, steps_per_tick=steps), "captured": TaskEnv(sim, cpg, task, steps_per_tick=steps, capture=True)}
    for env in envs.values():
        env.reset()
        window(lambda k: env.step(action), 10)
    env_us = {name: [] for name in envs}
    for _ in range(7):
        for name, env in envs.items():
            env_us[name].append(window(lambda k: env.step(action), 10))
    env_us = {name: statistics.median(v) for name, v in env_us.items()}

# the one-read-one-write model of an update: per world 2 n_act forces and velocities, n_q angles, 96 sensor floats read and the
# observation row written
bytes_per_world = 4 * (2 * task.n_act + task.n_q + 96 + task.obs_width)
result = dict(worlds=n, n_act=task.n_act, n_q=task.n_q, ticks_compared=args.ticks, calls_per_window=args.calls, agreement=agreement,
              agreement_ok=ok, control_steps=steps, cpg_step_us=bare_us, kernel_in_graph_us=graph_us, env_step_us=env_us,
              model_bytes=bytes_per_world * n, model_gb_per_s_in_graph=bytes_per_world * n / graph_us * 1e-3, variants={})
for name, us in times.items():
    med = statistics.median(us)
    result["variants"][name] = dict(median=med, min=min(us), max=max(us), windows=len(us), share_of_control_tick=med / bare_us)
    print(f"{name:8s}: {med:8.1f} us per update (min {min(us):.1f}, max {max(us):.1f}, {len(us)} windows of {args.calls}); "
          f"{100 * med / bare_us:.2f} % of cpg.step({steps})")
print(f"kernel, {args.calls} updates replayed as one captured graph: {graph_us:.2f} us per update; {100 * graph_us / bare_us:.3f} % of cpg.step({steps}); "
      f"{result['model_gb_per_s_in_graph']:.0f} GB/s of the {bytes_per_world * n / 1e6:.2f} MB one-read-one-write model")
print(f"cpg.step({steps}) alone {bare_us:.1f} us; TaskEnv.step eager {env_us['eager']:.1f} us, captured {env_us['captured']:.1f} us")
print(f"kernel against torch over {args.ticks} ticks of a walk: " + ", ".join(f"{k} {v}" for k, v in agreement.items())
      + f" ({'equal' if ok else 'NOT EQUAL'})")
print(json.dumps(result))
if args.out is not None:
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(result, indent=1) + "\n")
task.close()
