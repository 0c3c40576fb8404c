"""Time ``RuleBasedController.advance(20)`` on the GPU: 4096 worlds x 20 steps x 48 columns, against ``TurningCPG.advance(20)`` in the
same run (it writes the same 15.7 MB table: the yardstick), against the same rule written with torch operations issued per physics
step, and against the 20-step control tick it belongs to (``ctl.step(20)``).

The flavours alternate in the same process after a warm-up; each is timed by device events over windows of --calls calls until at
least --seconds have been measured.  The recurrence alone (phase A of the kernel) is timed on a second handle made through the C
ABI with ONE position column and no adhesion columns, whose row expansion is 1 / 48 of the work.  Before the timing the kernel and
the torch flavour advance the same --ticks ticks and their rows and counters are compared.
Results go to stdout and, as JSON, to --out (recorded by hand in profiles/rules_summary.md).  Needs an MI355X: no fallback."""
import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
from flygym_amd import HIPSimulation, _native, make_model
from flygym_amd.controllers import RuleBasedController, TurningCPG, _RulesParams

parser = argparse.ArgumentParser()
parser.add_argument("--worlds", type=int, default=4096)
parser.add_argument("--ticks", type=int, default=60)
parser.add_argument("--calls", type=int, default=50)
parser.add_argument("--seconds", type=float, default=0.5)
parser.add_argument("--control-steps", type=int, default=20)
parser.add_argument("--out", type=Path, default=None)
args = parser.parse_args()
if not torch.cuda.is_available():
    sys.exit("rules_bench.py measures on the GPU and found none")

n, steps = args.worlds, args.control_steps
ADHESION = (20.0, 1.0)
fly, world, _ = make_model()
sim = HIPSimulation(world, n_worlds=n, device=0)
sim.set_leg_adhesion_states(fly.name, np.ones((n, 6), dtype=np.float32))
sim.warmup()
dev = sim.device
ctl = RuleBasedController(sim, fly.name, adhesion=ADHESION, seed=3)
cpg = TurningCPG(sim, fly.name, adhesion=ADHESION)
M = 0xFFFFFFFF


def hash32(x):
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & M
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & M                          # (int64 products wrap; the low 32 bits are the uint32 product's)
    return x ^ (x >> 16)


class TorchRule:
    """One physics step of the rule in torch operations on tensors of its own (the arithmetic of include/nmf.h, operation by
    operation), writing one row of a table."""

    def __init__(self):
        t = lambda a, dtype: torch.as_tensor(np.asarray(a), device=dev).to(dtype)
        self.P, self.n_bins, self.n_pos = ctl.period_steps, ctl.n_bins, len(ctl.actuated_dofs)
        self.cyc, self.lod, self.cols = t(ctl.cycle, torch.float32), t(ctl.leg_of_dof, torch.int64), torch.arange(self.n_pos, device=dev)
        self.start, self.swing, self.W = t(ctl.start_bin, torch.int64), t(ctl.swing_steps, torch.int64), t(ctl.weights, torch.float32)
        self.rest = self.cyc[self.start[self.lod], self.cols]
        self.stance_steps = (self.P - self.swing).to(torch.float32)
        self.k = torch.zeros((n, 6), dtype=torch.int64, device=dev)
        self.stepping = torch.zeros((n, 6), dtype=torch.bool, device=dev)
        self.amp = torch.ones((n, 6), dtype=torch.float32, device=dev)
        self.ticks = torch.zeros(n, dtype=torch.int64, device=dev)
        self.world_key = ((ctl.first_world + torch.arange(n, device=dev, dtype=torch.int64)) * 0x9E3779B9) & M
        self.side = torch.tensor([0, 0, 0, 1, 1, 1], device=dev)
        self.on, self.off = (torch.tensor(v, dtype=torch.float32, device=dev) for v in ADHESION)
        self.table = torch.zeros((n, ctl.table_steps, self.n_pos + 6), dtype=torch.float32, device=dev)

    def step(self, drive6, latch, s):
        k, P = self.k, self.P
        x = (k * self.n_bins).double() / float(P)
        i0 = torch.floor(x)
        f = (x - i0).float()[:, self.lod]
        b0 = (self.start[None, :] + i0.long()) % self.n_bins
        b1 = (b0 + 1) % self.n_bins
        c = (1 - f) * self.cyc[b0[:, self.lod], self.cols] + f * self.cyc[b1[:, self.lod], self.cols]
        self.table[:, s, :self.n_pos] = self.rest + self.amp[:, self.lod] * (c - self.rest)
        swinging = (k > 0) & (k < self.swing)
        self.table[:, s, self.n_pos:] = torch.where(swinging, self.off, self.on)
        p = torch.clamp(k - self.swing, min=0).float() / self.stance_steps
        r1, r2, r3 = (torch.zeros((n, 6), dtype=torch.float32, device=dev) for _ in range(3))
        for src in range(6):
            ps = p[:, src:src + 1]
            r1 = r1 + torch.where(swinging[:, src:src + 1], self.W[0, src][None, :], 0.0)
            r2 = torch.where(ps > 0, r2 + self.W[1, src][None, :] * (1 - ps), r2)
            r3 = torch.where(ps > 0, r3 + self.W[2, src][None, :] * ps, r3)
        score = (r1 + r2) + r3
        best = score.max(dim=1).values
        below = best - best.abs() * ctl._params.margin
        thr = torch.where(below > 0, below, 0.0)
        driven = drive6 != 0
        eligible = (score >= thr[:, None]) & (score > 0) & ~self.stepping & driven
        fallback = ~self.stepping.any(dim=1) & ~eligible.any(dim=1)
        eligible = torch.where(fallback[:, None], driven, eligible)
        count = eligible.sum(dim=1)
        u = hash32((ctl.seed ^ self.world_key) ^ ((self.ticks * 0x85EBCA6B) & M) ^ ((11 * 0xC2B2AE35) & M))
        j = (u * count) >> 32
        chosen = eligible & (torch.cumsum(eligible, dim=1) - 1 == j[:, None])
        self.stepping = self.stepping | chosen
        self.amp = torch.where(chosen, latch, self.amp)
        k = torch.where(self.stepping, k + 1, k)
        done = k == P
        self.k = torch.where(done, 0, k)
        self.stepping = self.stepping & ~done
        self.ticks = self.ticks + 1

    def advance(self, drive, n_steps):
        drive6 = drive[:, self.side]
        latch = torch.where(drive6.abs() > ctl._params.max_amplitude, ctl._params.max_amplitude, drive6.abs())
        for s in range(n_steps):
            self.step(drive6, latch, s)
        return self.table


def window(fn, calls):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for k in range(calls):
        fn(k)
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / calls          # microseconds per call


# the recurrence alone: a handle of the C ABI with one position column and no adhesion columns
lib = _native.lib()
thin = _RulesParams.from_buffer_copy(ctl._params)
thin.n_pos, thin.adhesion = 1, 0
cycle1 = np.ascontiguousarray(ctl.cycle[:, :1], dtype=np.float32)
legs1 = np.ascontiguousarray(ctl.leg_of_dof[:1], dtype=np.int32)
thin_h = lib.nmf_rules_create(sim._batch_h, ctypes.byref(thin), cycle1.ctypes.data, legs1.ctypes.data, ctl.start_bin.ctypes.data,
                              ctl.swing_steps.ctypes.data, ctl.weights.ctypes.data)
if not thin_h:
    sys.exit(lib.nmf_last_error().decode())
thin_table = torch.zeros((n, ctl.table_steps, 1), dtype=torch.float32, device=dev)

rule = TorchRule()
rng = np.random.default_rng(1)
differ = dict(rows=0, counter=0, stepping=0, amplitude=0)
for tick in range(args.ticks):                         # both flavours advance the same ticks under the same changing drives
    drive = torch.as_tensor(rng.uniform(0.3, 1.8, (n, 2)).astype(np.float32), device=dev)
    drive[torch.as_tensor(rng.random(n) < 0.1, device=dev)] = 0
    ctl.set_drive(drive)
    got = ctl.advance(steps)[:, :steps]
    want = rule.advance(drive, steps)[:, :steps]
    differ["rows"] += int((got != want).sum())
    differ["counter"] += int((ctl.counter != rule.k).sum())
    differ["stepping"] += int((ctl.stepping.bool() != rule.stepping).sum())
    differ["amplitude"] += int((ctl.amplitude != rule.amp).sum())
torch.cuda.synchronize()
started = int(ctl.stepping.sum())
ok = all(v == 0 for v in differ.values())
ctl.set_drive(np.ones((n, 2), dtype=np.float32))
ones = torch.ones((n, 2), dtype=torch.float32, device=dev)

variants = {"rules": (lambda k: ctl.advance(steps), args.calls), "cpg": (lambda k: cpg.advance(steps), args.calls),
            "rules, recurrence alone": (lambda k: _native.check(lib.nmf_rules_advance(thin_h, steps, thin_table.data_ptr(), ctl.table_steps,
                                                                                     sim._stream())), args.calls),
            "torch": (lambda k: rule.advance(ones, steps), 2)}
for fn, calls in variants.values():                    # warm-up of every timed shape
    window(fn, calls)
times = {name: [] for name in variants}
total = {name: 0.0 for name in variants}
while min(total[name] for name in variants if name != "torch") < args.seconds * 1e6:    # alternated: a window of each in turn
    for name, (fn, calls) in variants.items():
        if name == "torch" and total[name] >= args.seconds * 1e6:
            continue                                   # (a torch advance is a thousand launches: its share of the time is capped)
        us = window(fn, calls)
        times[name].append(us)
        total[name] += us * calls

# the launches without the host between the calls: --calls advances captured as one graph (one chain), timed per replay
graph_us = {}
for name in ("rules", "cpg", "rules, recurrence alone"):
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for k in range(args.calls):
            variants[name][0](k)
    for _ in range(3):
        window(lambda k: graph.replay(), 5)
    graph_us[name] = statistics.median(window(lambda k: graph.replay(), 5) for _ in range(15)) / args.calls

for _ in range(3):
    window(lambda k: ctl.step(steps), 10)
tick_us = statistics.median(window(lambda k: ctl.step(steps), 10) for _ in range(7))
cpg_tick_us = statistics.median(window(lambda k: cpg.step(steps), 10) for _ in range(7))

table_mb = n * steps * ctl.n_act * 4 / 1e6
result = dict(worlds=n, control_steps=steps, columns=ctl.n_act, table_megabytes=table_mb, ticks_compared=args.ticks, differ=differ,
              agreement_ok=ok, legs_stepping_after_comparison=started, period_steps=ctl.period_steps, control_tick_us=tick_us,
              cpg_control_tick_us=cpg_tick_us, in_graph_us=graph_us, variants={})
for name, us in times.items():
    med = statistics.median(us)
    result["variants"][name] = dict(median=med, min=min(us), max=max(us), windows=len(us), calls_per_window=variants[name][1],
                                    share_of_control_tick=med / tick_us)
    print(f"{name:24s}: {med:9.1f} us per advance({steps}) (min {min(us):.1f}, max {max(us):.1f}, {len(us)} windows of {variants[name][1]}); "
          f"{100 * med / tick_us:.2f} % of the control tick")
for name, us in graph_us.items():
    print(f"{name:24s}: {us:9.2f} us per advance({steps}) as {args.calls} launches replayed in one captured graph; "
          f"{100 * us / tick_us:.2f} % of the control tick; {table_mb / us if 'alone' not in name else 0:.2f} TB/s of table written")
print(f"control tick ctl.step({steps}): {tick_us:.1f} us; cpg.step({steps}): {cpg_tick_us:.1f} us; table {table_mb:.1f} MB")
print(f"kernel against torch after {args.ticks} ticks: entries that differ {differ} ({'equal' if ok else 'NOT EQUAL'}); "
      f"{started} legs stepping at the end")
print(json.dumps(result))
if args.out is not None:
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(result, indent=1) + "\n")
lib.nmf_rules_destroy(thin_h)
ctl.close(); cpg.close()
sys.exit(0 if ok else 1)
