"""Time ``PlumeNavigator.update`` on the GPU: 4096 worlds, against the same rule written with torch operations on the same data
(the counter-based draws in int64 arithmetic, the filters, the state logic and the drive table as tensor operations), and against
the 20-step control tick it belongs to (``cpg.step(20)`` + ``update``).

The two flavours alternate in the same process after a warm-up; each is timed by device events over windows of --calls calls until
at least --seconds have been measured: calls issued from Python back to back, so a figure near 10 us is as much the host's issue
rate as the kernel.  The kernel is therefore also timed as --calls updates captured into one graph and replayed.  Before the timing
both flavours follow --ticks ticks of a real walk through per-world plumes and their states are compared: every operation of the
rule is a single IEEE float32 operation in both, so they must be equal.
Results go to stdout and, as JSON, to --out (recorded by hand in profiles/navigator_summary.md).  Needs an MI355X: no fallback."""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
from flygym_amd import HIPSimulation, make_model
from flygym_amd.controllers import PlumeNavigator, TurningCPG
from flygym_amd.sensors import OdorPlume

parser = argparse.ArgumentParser()
parser.add_argument("--worlds", type=int, default=4096)
parser.add_argument("--ticks", type=int, default=150)
parser.add_argument("--calls", type=int, default=50)
parser.add_argument("--seconds", type=float, default=0.5)
parser.add_argument("--control-steps", type=int, default=20)
parser.add_argument("--out", type=Path, default=None)
args = parser.parse_args()
if not torch.cuda.is_available():
    sys.exit("navigator_bench.py measures on the GPU and found none")

n, steps = args.worlds, args.control_steps
fly, world, _ = make_model()
sim = HIPSimulation(world, n_worlds=n, device=0)
sim.set_leg_adhesion_states(fly.name, np.ones((n, 6), dtype=np.float32))
sim.warmup()
dev = sim.device
tick_s = steps * sim.timestep
# rates ten times Demir et al.'s so that the --ticks ticks of the comparison see every transition many times
nav = PlumeNavigator(sim, fly.name, tick_s=tick_s, threshold=0.02, seed=3, stop_rate=(7.8, -6.1), walk_rate=(2.9, 4.1), turn_rate=13.3,
                     turn_duration=0.05)
P = nav._params
nseg, M = sim.model.nseg, 0xFFFFFFFF
f = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)
rows = torch.tensor([list(P.walk_drive), list(P.stop_drive), list(P.turn_drive), list(P.turn_drive)[::-1]], dtype=torch.float32, device=dev)
world_key = ((P.first_world + torch.arange(n, device=dev, dtype=torch.int64)) * 0x9E3779B9) & M
zero = f(0.0)


def hash32(x):
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & M
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & M                          # (int64 products wrap; the low 32 bits are the uint32 product's)
    return x ^ (x >> 16)


class TorchRule:
    """The update in torch operations on tensors of its own (float32 throughout, each operation rounded on its own as in the kernel)."""

    def __init__(self):
        z = lambda dtype: torch.zeros(n, dtype=dtype, device=dev)
        self.state, self.remaining, self.above = z(torch.int32), z(torch.int32), z(torch.bool)
        self.k_stop, self.k_walk, self.freq = z(torch.float32), z(torch.float32), z(torch.float32)
        self.ticks, self.encounters = z(torch.int64), z(torch.int32)
        self.drive = torch.ones((n, 2), dtype=torch.float32, device=dev)

    def update(self, odor, wind, out):
        I = odor[:, P.odor_dim]
        qw, qx, qy, qz = sim.field("seg_xquat").view(n, nseg, 4)[:, nav.root_seg].unbind(dim=1)
        now = (I[:, 2] + I[:, 3]) > P.threshold
        e = now & ~self.above
        ef = e.to(torch.float32)
        k_stop = self.k_stop * P.decay_stop + ef
        k_walk = self.k_walk * P.decay_walk + ef
        freq = self.freq * P.decay_freq + torch.where(e, f(P.inv_tau_freq), zero)
        ax = 1 - 2 * (qy * qy + qz * qz)
        ay = 2 * (qx * qy + qw * qz)
        up_left = (ay * wind[:, 0] - ax * wind[:, 1]) > 0
        key = (P.seed ^ world_key) ^ ((self.ticks * 0x85EBCA6B) & M)
        u0, u1, u2 = ((hash32(key ^ ((m * 0xC2B2AE35) & M)) >> 8).to(torch.float32) * 2.0 ** -24 for m in (8, 9, 10))
        p_stop = torch.clamp(f(P.dt) * (P.lambda_ws0 + P.dlambda_ws * k_stop), 0, 1)
        p_walk = torch.clamp(f(P.dt) * (P.lambda_sw0 + P.dlambda_sw * k_walk), 0, 1)
        p_turn = torch.clamp(f(P.dt) * f(P.lambda_turn), 0, 1)
        p_up = torch.clamp(P.p_up0 + P.up_gain * freq, P.p_up_min, P.p_up_max)
        walking, stopped = self.state == 0, self.state == 1
        turning = ~walking & ~stopped
        stop = walking & (u0 < p_stop)
        decided = walking & ~stop & (u1 < p_turn)
        side = torch.where((u2 < p_up) == up_left, 2, 3).to(torch.int32)
        remaining = torch.where(decided, P.turn_ticks, torch.where(turning, self.remaining - 1, self.remaining)).to(torch.int32)
        nxt = torch.where(stop, 1, torch.where(decided, side, self.state))
        nxt = torch.where(stopped & (u0 < p_walk), 0, nxt)
        nxt = torch.where(turning & (remaining <= 0), 0, nxt).to(torch.int32)
        self.state, self.remaining, self.above = nxt, remaining, now
        self.k_stop, self.k_walk, self.freq = k_stop, k_walk, freq
        self.ticks = self.ticks + 1
        self.encounters = self.encounters + e.to(torch.int32)
        out.copy_(rows[nxt.long()])


def window(fn, calls):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for k in range(calls):
        fn(k)
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / calls          # microseconds per call


rule = TorchRule()
plume = OdorPlume(sim, fly.name, grid=(48, 80), cell_size=0.5, origin=(-8.0, -12.0), source=(10.0, 0.0, 1.0, 1.0), mean_wind=(-60.0, 0.0),
                  wind_tau=0.5, wind_sigma=60.0, diffusivity=1.0, tick_s=tick_s, seed=1)
buf = torch.zeros((n, 1, 4), dtype=torch.float32, device=dev)
with plume, TurningCPG(sim, fly.name) as cpg:
    plume.advance(int(round(0.4 / tick_s)))
    seen = torch.zeros(4, dtype=torch.int64, device=dev)
    for _ in range(args.ticks):                        # both flavours follow the same walk; the kernel's drive steers it
        plume.advance()
        plume.get_odor_intensities(out=buf)
        rule.update(buf, plume.wind, rule.drive)
        nav.update(buf, plume.wind, out=cpg.drive)
        seen += torch.bincount(nav.state.long(), minlength=4)
        cpg.step(steps)
    torch.cuda.synchronize()
    agreement = dict(state=int((nav.state != rule.state).sum()), remaining=int((nav.remaining != rule.remaining).sum()),
                     encounters=int((nav.encounters != rule.encounters).sum()), drive=int((cpg.drive != rule.drive).any(dim=1).sum()),
                     k_stop=float((nav.k_stop - rule.k_stop).abs().max()), k_walk=float((nav.k_walk - rule.k_walk).abs().max()),
                     freq=float((nav.freq - rule.freq).abs().max()), total_encounters=int(nav.encounters.sum()),
                     world_ticks_per_state=seen.tolist())
    ok = all(agreement[k] == 0 for k in ("state", "remaining", "encounters", "drive", "k_stop", "k_walk", "freq")) and min(seen.tolist()) > 0

    variants = {"kernel": lambda k: nav.update(buf, plume.wind, out=cpg.drive), "torch": lambda k: rule.update(buf, plume.wind, rule.drive)}
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
            nav.update(buf, plume.wind, out=cpg.drive)
    for _ in range(3):
        window(lambda k: graph.replay(), 10)
    graph_us = statistics.median(window(lambda k: graph.replay(), 10) for _ in range(15)) / args.calls

    def tick(k):
        nav.update(buf, plume.wind, out=cpg.drive)
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
print(f"kernel against torch after {args.ticks} ticks of a walk: " + ", ".join(f"{k} {v}" for k, v in agreement.items())
      + f" ({'equal' if ok else 'NOT EQUAL'})")
print(json.dumps(result))
if args.out is not None:
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(result, indent=1) + "\n")
nav.close()
sys.exit(0 if ok else 1)
