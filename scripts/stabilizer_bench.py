"""Time ``HeadStabilizer.update`` on the GPU: 4096 worlds, the default 48 -> 32 -> 32 -> 2 network, against the same rule written
with torch operations on the same data (a gather, the standardisation, the contact flags, three ``linear``s, two ReLUs, a clamp and
a scatter), and against the 20-step control tick it belongs to (``update`` + ``cpg.step(20)``).

The two flavours alternate in the same process after a warm-up; each is timed by device events over windows of --calls calls until
at least --seconds have been measured: calls issued from Python back to back, so a figure near 10 us is as much the host's issue
rate as the kernel.  The kernel is therefore also timed as --calls updates captured into one graph and replayed.  Before the timing
the flies walk --ticks ticks and the two flavours' outputs are compared: torch's ``linear`` sums in another order, so they agree to
rounding, not bit for bit (the kernel's bits are pinned by tests/test_stabilizer_gpu.py).
Results go to stdout and, as JSON, to --out (recorded by hand in profiles/stabilizer_summary.md).  Needs an MI355X: no fallback."""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
from flygym_amd import HIPSimulation, make_model
from flygym_amd.controllers import HeadStabilizer, TurningCPG

parser = argparse.ArgumentParser()
parser.add_argument("--worlds", type=int, default=4096)
parser.add_argument("--ticks", type=int, default=50)
parser.add_argument("--calls", type=int, default=50)
parser.add_argument("--seconds", type=float, default=0.5)
parser.add_argument("--control-steps", type=int, default=20)
parser.add_argument("--out", type=Path, default=None)
args = parser.parse_args()
if not torch.cuda.is_available():
    sys.exit("stabilizer_bench.py measures on the GPU and found none")

n, steps = args.worlds, args.control_steps
fly, world, _ = make_model()
sim = HIPSimulation(world, n_worlds=n, device=0)
sim.set_leg_adhesion_states(fly.name, np.ones((n, 6), dtype=np.float32))
sim.warmup()
dev = sim.device
rng = np.random.default_rng(0)
sizes = [48, 32, 32, 2]
layers = [(rng.normal(0, np.sqrt(2.0 / a), (b, a)).astype(np.float32), rng.normal(0, 0.1, b).astype(np.float32)) for a, b in zip(sizes[:-1], sizes[1:])]
layers[-1] = (0.1 * layers[-1][0], layers[-1][1])      # (outputs of a few tenths of a radian: most stay inside the limits)
mean, std = rng.normal(0, 0.5, 42).astype(np.float32), rng.uniform(0.5, 1.5, 42).astype(np.float32)
limits = (-0.3, 0.3)
stab = HeadStabilizer(sim, fly.name, layers, input_mean=mean, input_std=std, limits=limits, drive_actuators=False)

f = lambda a: torch.as_tensor(a, device=dev)
cols = f(7 + stab._dof.astype(np.int64))
t_mean, t_inv = f(mean), f(stab._inv_std)
t_layers = [(f(W), f(b)) for W, b in layers]
thr2 = f(stab.thr2)
scratch_ctrl = torch.zeros((n, sim.model.nu), dtype=torch.float32, device=dev)   # the torch rule's scatter target
act = f(np.array([0, 1], dtype=np.int64))
out_torch = torch.zeros((n, 2), dtype=torch.float32, device=dev)


def torch_rule():
    x = (sim.field("qpos")[:, cols] - t_mean) * t_inv
    sd = sim.field("sensordata").view(n, 6, 16)
    m = sd[:, :, 1] * sd[:, :, 1] + sd[:, :, 2] * sd[:, :, 2] + sd[:, :, 3] * sd[:, :, 3]
    h = torch.cat([x, ((sd[:, :, 0] > 0) & (m > thr2)).to(torch.float32)], dim=1)
    h = torch.relu(torch.nn.functional.linear(h, *t_layers[0]))
    h = torch.relu(torch.nn.functional.linear(h, *t_layers[1]))
    y = torch.clamp(torch.nn.functional.linear(h, *t_layers[2]), *limits)
    out_torch.copy_(y)
    scratch_ctrl[:, act] = y


def window(fn, calls):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for k in range(calls):
        fn(k)
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / calls          # microseconds per call


with TurningCPG(sim, fly.name) as cpg:
    worst, clamped, flags = 0.0, 0, torch.zeros(6, dtype=torch.int64, device=dev)
    for _ in range(args.ticks):
        stab.update()
        torch_rule()
        worst = max(worst, float((stab.output - out_torch).abs().max()))
        clamped += int(((stab.output == limits[0]) | (stab.output == limits[1])).sum())
        flags += (sim.field("sensordata").view(n, 6, 16)[:, :, 0] > 0).sum(dim=0)
        cpg.step(steps)
    torch.cuda.synchronize()
    agreement = dict(largest_difference=worst, clamped_outputs=clamped, outputs=2 * n * args.ticks, leg_contacts_seen=flags.tolist())
    ok = worst < 1e-4 and clamped < agreement["outputs"] // 2

    variants = {"kernel": lambda k: stab.update(), "torch": lambda k: torch_rule()}
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
            stab.update()
    for _ in range(3):
        window(lambda k: graph.replay(), 10)
    graph_us = statistics.median(window(lambda k: graph.replay(), 10) for _ in range(15)) / args.calls

    def tick(k):
        stab.update()
        cpg.step(steps)

    for _ in range(3):
        window(tick, 10)
    tick_us = statistics.median(window(tick, 10) for _ in range(7))
    bare_us = statistics.median(window(lambda k: cpg.step(steps), 10) for _ in range(7))

result = dict(worlds=n, ticks_compared=args.ticks, calls_per_window=args.calls, agreement=agreement, agreement_ok=ok, control_steps=steps,
              control_tick_us=tick_us, tick_without_update_us=bare_us, kernel_in_graph_us=graph_us, variants={})
for name, us in times.items():
    med = statistics.median(us)
    result["variants"][name] = dict(median=med, min=min(us), max=max(us), windows=len(us), share_of_control_tick=med / tick_us)
    print(f"{name:8s}: {med:8.1f} us per update (min {min(us):.1f}, max {max(us):.1f}, {len(us)} windows of {args.calls}); "
          f"{100 * med / tick_us:.2f} % of the control tick")
print(f"kernel, {args.calls} updates replayed as one captured graph: {graph_us:.2f} us per update; {100 * graph_us / tick_us:.2f} % of the control tick")
print(f"control tick (update + cpg.step({steps})): {tick_us:.1f} us; cpg.step({steps}) alone {bare_us:.1f} us")
print(f"kernel against torch over {args.ticks} ticks of a walk: " + ", ".join(f"{k} {v}" for k, v in agreement.items())
      + f" ({'agree to rounding' if ok else 'DO NOT AGREE'})")
print(json.dumps(result))
if args.out is not None:
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(result, indent=1) + "\n")
stab.close()
sys.exit(0 if ok else 1)
