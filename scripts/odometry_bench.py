"""Time ``PathIntegrator.update`` on the GPU: 4096 worlds, against the same rule written with torch operations on the same data
(a rolling window of totals kept as a ring tensor, float64 where the kernel is float64), and against the 20-step control tick it
belongs to (``cpg.step(20)`` + ``update``).

The two flavours alternate in the same process after a warm-up; each is timed by device events over windows of --calls calls until
at least --seconds have been measured.  Before the timing both flavours follow --window + 40 ticks of a real walk (200 at the default) and their
states are compared.  Results go to stdout and, as JSON, to --out (recorded by hand in profiles/odometry_summary.md).  Needs an MI355X: no
fallback."""
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
from flygym_amd.sensors import PathIntegrator

parser = argparse.ArgumentParser()
parser.add_argument("--worlds", type=int, default=4096)
parser.add_argument("--window", type=int, default=160)
parser.add_argument("--calls", type=int, default=50)
parser.add_argument("--seconds", type=float, default=0.5)
parser.add_argument("--control-steps", type=int, default=20)
parser.add_argument("--out", type=Path, default=None)
args = parser.parse_args()
if not torch.cuda.is_available():
    sys.exit("odometry_bench.py measures on the GPU and found none")

n, W = args.worlds, args.window
fly, world, _ = make_model()
sim = HIPSimulation(world, n_worlds=n, device=0)
sim.set_leg_adhesion_states(fly.name, np.ones((n, 6), dtype=np.float32))
sim.warmup()
dev = sim.device
rng = np.random.default_rng(0)
coef = np.concatenate([[0.2, 0.1, 0.15, -0.2, -0.1, -0.15], np.full(6, 1.0 / 6.0), [0.01, 0.02]])
odo = PathIntegrator(sim, fly.name, window=W, contact_force_thresholds=(0.5, 1.0, 3.0), coefficients=coef)
nseg = sim.model.nseg
tips = torch.as_tensor(odo.tip_seg.astype(np.int64), device=dev)
thr2 = torch.as_tensor(odo.contact_force_thresholds, device=dev) ** 2
thr0 = thr2 == 0
c_h, c_d = (torch.as_tensor(coef[a:b], device=dev) for a, b in ((0, 6), (6, 12)))


class TorchRule:
    """The update in torch operations: the state is a set of tensors, the ring is indexed with a host-side cursor (so this flavour,
    unlike the kernel, cannot replay from a captured graph or reset single worlds)."""

    def __init__(self):
        z = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=dev)
        self.k = 0
        self.xprev, self.cprev = z(n, 6, dtype=torch.float32), z(n, 6, dtype=torch.bool)
        self.total, self.ring, self.win = z(n, 6), z(W, n, 6), z(n, 6)
        self.heading, self.position, self.home = z(n), z(n, 2), z(n, 2)

    def update(self):
        xpos = sim.field("seg_xpos").view(n, nseg, 3)
        qw, qx, qy, qz = sim.field("seg_xquat").view(n, nseg, 4)[:, odo.root_seg].unbind(dim=1)
        axis = torch.stack([1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy + qw * qz), 2 * (qx * qz - qw * qy)], dim=1)
        x = ((xpos[:, tips] - xpos[:, odo.root_seg, None]) * axis[:, None]).sum(dim=2)
        sd = sim.field("sensordata").view(n, 6, 16)
        c = (sd[..., 0] > 0) & (thr0 | ((sd[..., 1:4] ** 2).sum(dim=2) > thr2))
        if self.k > 0:
            self.total += torch.where(c & self.cprev, (self.xprev - x).to(torch.float64), 0.0)
        slot = self.k % W
        self.win = self.total - self.ring[slot]
        self.ring[slot] = self.total
        if self.k >= W:
            self.heading = torch.remainder(self.heading + (coef[12] + self.win @ c_h) / W + np.pi, 2 * np.pi) - np.pi
        cs, sn = torch.cos(self.heading), torch.sin(self.heading)
        if self.k >= W:
            self.position = self.position + ((coef[13] + self.win @ c_d) / W)[:, None] * torch.stack([cs, sn], dim=1)
        px, py = self.position.unbind(dim=1)
        self.home = torch.stack([-(cs * px + sn * py), -(-sn * px + cs * py)], dim=1)
        self.xprev, self.cprev = x, c
        self.k += 1


def window(fn, calls):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for k in range(calls):
        fn(k)
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / calls          # microseconds per call


steps = args.control_steps
rule = TorchRule()
with TurningCPG(sim, fly.name) as cpg:
    cpg.set_drive(rng.uniform(0.4, 1.2, (n, 2)).astype(np.float32))
    for _ in range(W + 40):                            # both flavours follow the same walk, past the first window
        cpg.step(steps)
        odo.update()
        rule.update()
    torch.cuda.synchronize()
    agreement = dict(total=float((odo.stride_total - rule.total).abs().max()), window=float((odo.window_strides - rule.win).abs().max()),
                     heading=float((torch.remainder(odo.heading - rule.heading + np.pi, 2 * np.pi) - np.pi).abs().max()),
                     position=float((odo.position - rule.position).abs().max()), home=float((odo.home - rule.home).abs().max()),
                     path=float(torch.linalg.norm(odo.position, dim=1).mean()))
    # the torch flavour sums the three products in another order and takes torch's sine and cosine: float32 roundings of
    # coordinates of a few mm per update, W + 40 updates
    ok = agreement["total"] < 1e-3 and agreement["heading"] < 1e-4 and agreement["position"] < 1e-3

    variants = {"kernel": lambda k: odo.update(), "torch": lambda k: rule.update()}
    for fn in variants.values():                       # warm-up of every timed shape
        window(fn, args.calls)
    times = {name: [] for name in variants}
    total = {name: 0.0 for name in variants}
    while min(total.values()) < args.seconds * 1e6:    # alternated: a window of each in turn
        for name, fn in variants.items():
            us = window(fn, args.calls)
            times[name].append(us)
            total[name] += us * args.calls

    def tick(k):
        cpg.step(steps)
        odo.update()

    for _ in range(3):
        window(tick, 10)
    tick_us = statistics.median(window(tick, 10) for _ in range(7))
    bare_us = statistics.median(window(lambda k: cpg.step(steps), 10) for _ in range(7))

result = dict(worlds=n, window=W, calls_per_window=args.calls, agreement=agreement, agreement_ok=ok, control_steps=steps,
              control_tick_us=tick_us, tick_without_update_us=bare_us, variants={})
for name, us in times.items():
    med = statistics.median(us)
    result["variants"][name] = dict(median=med, min=min(us), max=max(us), windows=len(us), share_of_control_tick=med / tick_us)
    print(f"{name:8s}: {med:8.1f} us per update (min {min(us):.1f}, max {max(us):.1f}, {len(us)} windows of {args.calls}); "
          f"{100 * med / tick_us:.2f} % of the control tick")
print(f"control tick (cpg.step({steps}) + update): {tick_us:.1f} us; cpg.step({steps}) alone {bare_us:.1f} us")
print("kernel against torch after the walk: max |difference| " + ", ".join(f"{k} {v:.2e}" for k, v in agreement.items() if k != "path")
      + f" (mean estimated distance {agreement['path']:.3f}; {'within' if ok else 'OUTSIDE'} the tolerance)")
print(json.dumps(result))
if args.out is not None:
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(result, indent=1) + "\n")
odo.close()
sys.exit(0 if ok else 1)
