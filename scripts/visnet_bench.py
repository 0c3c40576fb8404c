"""Time ``RetinotopicNetwork.update`` on the GPU: 4096 worlds x 2 eyes x 721 ommatidia with ``sensors.motion_pathway()`` (15
types, 54 taps), with 1 and 4 sub-steps, eager and inside a replayed graph, against the same rule written with torch operations
(gathers and temporaries per tap; it sums floats, so its results are compared within a tolerance), and against a 20-step control
tick with the eye renderer (``render_into`` -> ``update`` -> ``cpg.step(20)``).

The flavours alternate in the same process after a warm-up; each is timed by device events over windows of --calls calls until at
least --seconds have been measured.  The traffic model is one read of the readings plus one read and one write of the state,
n x 2 x n_omm x (8 + 8 C) bytes — 757 MB at 4096 worlds, more than the Infinity Cache holds; its rate is set against the 8 TB/s
HBM peak.  Results go to stdout and, as JSON, to --out (recorded by hand in profiles/visnet_summary.md).  Needs an MI355X: no
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
from flygym_amd.sensors import RetinotopicNetwork, motion_pathway
from flygym_amd.vision import EyeRenderer, Scene

parser = argparse.ArgumentParser()
parser.add_argument("--worlds", type=int, default=4096)
parser.add_argument("--calls", type=int, default=20)
parser.add_argument("--seconds", type=float, default=0.3)
parser.add_argument("--control-steps", type=int, default=20)
parser.add_argument("--out", type=Path, default=None)
args = parser.parse_args()
if not torch.cuda.is_available():
    sys.exit("visnet_bench.py measures on the GPU and found none")

HBM_PEAK = 8.0e12
n, steps = args.worlds, args.control_steps
fly, world, _ = make_model()
sim = HIPSimulation(world, n_worlds=n, device=0)
sim.set_leg_adhesion_states(fly.name, np.ones((n, 6), dtype=np.float32))
sim.warmup()
dev = sim.device
dt = steps * float(sim.timestep)
nets = {sub: RetinotopicNetwork(sim, fly.name, motion_pathway(), dt=dt, substeps=sub) for sub in (1, 4)}
net = nets[1]
n_omm, C, p = net.n_omm, net.n_types, net._params
rng = np.random.default_rng(0)


def readings():
    r = rng.uniform(0.0, 1.0, (n, 2, n_omm)).astype(np.float32)
    pale = net.retina.pale_mask != 0
    return torch.as_tensor(np.stack([np.where(pale, 0, r), np.where(pale, r, 0)], axis=-1).astype(np.float32), device=dev)


buffers = [readings() for _ in range(4)]
types = torch.as_tensor(net.types, device=dev)
table = torch.as_tensor(np.where(net.neighbours < 0, n_omm, net.neighbours).astype(np.int64), device=dev)      # (2, T, n_omm)
chains = [[] for _ in range(C)]
for e, (post, pre) in enumerate(net.edges.tolist()):
    chains[post] += [(pre, int(net.taps[k, 1]), float(net.tap_w[k])) for k in np.nonzero(net.taps[:, 0] == e)[0]]
t_v = {sub: torch.zeros((n, 2, C, n_omm), device=dev) for sub in nets}


def torch_rule(omm, sub):
    """The same rule in torch operations, state in place (float sums, no fixed point, no fresh branch)."""
    v = t_v[sub]
    a = torch.as_tensor(nets[sub].types[:, 3], device=dev)
    for _ in range(sub):
        r = torch.cat([v.clamp(min=0), torch.zeros((n, 2, C, 1), device=dev)], dim=-1)
        new = torch.empty_like(v)
        for c in range(C):
            s = types[c, 0] + types[c, 1] * omm[..., 0] + types[c, 2] * omm[..., 1]
            for pre, t, w in chains[c]:
                s = s + w * torch.stack([r[:, 0, pre][:, table[0, t]], r[:, 1, pre][:, table[1, t]]], dim=1)
            new[:, :, c] = v[:, :, c] + a[c] * (s - v[:, :, c])
        v.copy_(new)
    pooled = v.clamp(0, 4).mean(dim=-1)
    signal = ((pooled[:, 0] - pooled[:, 1]) * types[:, 4]).sum(dim=-1)
    g = p.gain * signal
    q = g / (1.0 + g.abs())
    o = torch.stack([1.0 - p.delta * q.clamp(min=0), 1.0 - p.delta * (-q).clamp(min=0)], dim=1)
    return pooled, signal, (p.base * o).clamp(p.drive_min, p.drive_max)


def window(fn, calls):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for k in range(calls):
        fn(k)
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / calls          # microseconds per call


graphs = {}
for sub, handle in nets.items():                          # one update on a fixed buffer, captured
    handle.update(buffers[0])
    torch.cuda.synchronize()
    graphs[sub] = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graphs[sub]):
        handle.update(buffers[0])

variants = {"kernel, substeps 1, same buffer": lambda k: nets[1].update(buffers[0]),
            "kernel, substeps 1, rotating": lambda k: nets[1].update(buffers[k % 4]),
            "kernel, substeps 1, replayed graph": lambda k: graphs[1].replay(),
            "kernel, substeps 4, same buffer": lambda k: nets[4].update(buffers[0]),
            "kernel, substeps 4, replayed graph": lambda k: graphs[4].replay(),
            "torch, substeps 1, same buffer": lambda k: torch_rule(buffers[0], 1)}
calls = {name: max(2, args.calls // 10) if name.startswith("torch") else args.calls for name in variants}
for name, fn in variants.items():                        # warm-up of every timed shape
    window(fn, calls[name])
times = {name: [] for name in variants}
total = {name: 0.0 for name in variants}
while min(total.values()) < args.seconds * 1e6:           # alternated: a window of each in turn
    for name, fn in variants.items():
        us = window(fn, calls[name])
        times[name].append(us)
        total[name] += us * calls[name]

# agreement: both flavours from the same state over a few ticks of new readings
net.reset()
net.update(buffers[0])
t_v[1].copy_(net.v)
for k in (1, 2, 3):
    net.update(buffers[k])
    pooled, signal, drive = torch_rule(buffers[k], 1)
torch.cuda.synchronize()
agreement = dict(v=float((net.v - t_v[1]).abs().max()), pooled=float((net.pooled - pooled).abs().max()),
                 signal=float((net.signal - signal).abs().max()), drive=float((net.drive - drive).abs().max()),
                 v_scale=float(net.v.abs().max()))
# the torch flavour contracts nothing but sums in another order and skips the 2^-16 rounding of the pooled terms
ok = agreement["v"] < 1e-5 and agreement["pooled"] < 3e-5 and agreement["signal"] < 3e-4 and agreement["drive"] < 3e-4 * p.gain

# the control tick the update is part of
eyes = EyeRenderer(sim, fly.name, scene=Scene(checker_size=2.0, ground_rgb=((0, 0, 0), (1, 1, 1))))
omm = buffers[1]
with TurningCPG(sim, fly.name) as cpg:
    def tick(k):
        eyes.render_into(omm)
        net.update(omm, out=cpg.drive)
        cpg.step(steps)

    for _ in range(3):
        window(tick, 10)
    tick_us = statistics.median(window(tick, 10) for _ in range(7))
    eye_us = statistics.median(window(lambda k: eyes.render_into(omm), 10) for _ in range(7))
    in_tick_us = statistics.median(window(lambda k: (eyes.render_into(omm), net.update(omm, out=cpg.drive)), 10)
                                   for _ in range(7)) - eye_us

model_bytes = n * 2 * n_omm * (8 + 8 * C)
result = dict(worlds=n, n_omm=n_omm, n_types=C, n_taps=int(len(net.taps)), model_bytes=model_bytes, agreement=agreement,
              agreement_ok=ok, control_steps=steps, control_tick_us=tick_us, eye_render_us=eye_us, update_after_eyes_us=in_tick_us,
              variants={})
for name, us in times.items():
    med = statistics.median(us)
    rate = model_bytes / (med * 1e-6)
    result["variants"][name] = dict(us=dict(median=med, min=min(us), max=max(us), windows=len(us), calls=calls[name]),
                                    model_tb_per_s=rate / 1e12, share_of_hbm_peak=rate / HBM_PEAK, share_of_control_tick=med / tick_us)
    print(f"{name:36s}: {med:9.1f} us per call (min {min(us):.1f}, max {max(us):.1f}, {len(us)} windows of {calls[name]}) = "
          f"{rate / 1e12:.2f} TB/s of the model's {model_bytes / 1e6:.1f} MB = {100 * rate / HBM_PEAK:.0f} % of the HBM peak; "
          f"{100 * med / tick_us:.2f} % of the control tick")
print(f"control tick (render_into + update + cpg.step({steps})): {tick_us:.1f} us; render_into alone {eye_us:.1f} us; "
      f"update right after the eye kernel adds {in_tick_us:.1f} us")
print(f"kernel against torch: max |difference| v {agreement['v']:.2e} (largest |v| {agreement['v_scale']:.2e}), pooled "
      f"{agreement['pooled']:.2e}, signal {agreement['signal']:.2e}, drive {agreement['drive']:.2e} ({'within' if ok else 'OUTSIDE'} the tolerance)")
print(json.dumps(result))
if args.out is not None:
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(result, indent=1) + "\n")
for handle in nets.values():
    handle.close()
sys.exit(0 if ok else 1)
