"""Time ``MotionDetectors.update`` on the GPU: 4096 worlds x 2 eyes x 721 ommatidia and the default retina's 2070 pairs, against
the same rule written with torch operations (several passes with temporaries; it sums floats, so its results are compared within a
tolerance), and against a 20-step control tick with the eye renderer (``render_into`` -> ``update`` -> ``cpg.step(20)``).

The two flavours alternate in the same process after a warm-up; each is timed by device events over windows of --calls calls until
at least --seconds have been measured.  The readings are 47 MB and the two filter states another 47 MB, less than the Infinity
Cache: "same buffer" re-reads one tensor (as the tick does, right after the eye kernel wrote it), "rotating" walks over eight
tensors (378 MB) — the state is the same 47 MB either way.  The traffic model is one read of the readings plus one read and one
write of the state, n x 2 x n_omm x (8 + 8 + 8) bytes; its rate is set against the 8 TB/s HBM peak.
Results go to stdout and, as JSON, to --out (recorded by hand in profiles/motion_summary.md).  Needs an MI355X: no fallback."""
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
from flygym_amd.sensors import MotionDetectors
from flygym_amd.vision import EyeRenderer, Scene

parser = argparse.ArgumentParser()
parser.add_argument("--worlds", type=int, default=4096)
parser.add_argument("--calls", type=int, default=50)
parser.add_argument("--seconds", type=float, default=0.5)
parser.add_argument("--control-steps", type=int, default=20)
parser.add_argument("--out", type=Path, default=None)
args = parser.parse_args()
if not torch.cuda.is_available():
    sys.exit("motion_bench.py measures on the GPU and found none")

HBM_PEAK = 8.0e12
n, steps = args.worlds, args.control_steps
fly, world, _ = make_model()
sim = HIPSimulation(world, n_worlds=n, device=0)
sim.set_leg_adhesion_states(fly.name, np.ones((n, 6), dtype=np.float32))
sim.warmup()
dev = sim.device
dt = steps * float(sim.timestep)
motion = MotionDetectors(sim, fly.name, dt=dt)
n_omm, n_pairs, p = motion.n_omm, motion.n_pairs, motion._params
rng = np.random.default_rng(0)


def readings():
    r = rng.uniform(0.0, 1.0, (n, 2, n_omm)).astype(np.float32)
    pale = motion.retina.pale_mask != 0
    return torch.as_tensor(np.stack([np.where(pale, 0, r), np.where(pale, r, 0)], axis=-1).astype(np.float32), device=dev)


buffers = [readings() for _ in range(8)]
pa = torch.as_tensor(motion.pairs[:, 0].astype(np.int64), device=dev)
pb = torch.as_tensor(motion.pairs[:, 1].astype(np.int64), device=dev)
wts = torch.as_tensor(motion.weights, device=dev)
sign = torch.tensor([-1.0 if f else 1.0 for f in motion.front_edge], device=dev)
t_fast, t_slow = torch.zeros((n, 2, n_omm), device=dev), torch.zeros((n, 2, n_omm), device=dev)


def torch_rule(omm):
    """The same rule in torch operations, state in place (float sums, no fixed point, no fresh branch)."""
    x = omm[..., 0] + omm[..., 1]
    t_fast.add_(p.a_fast * (x - t_fast))
    t_slow.add_(p.a_slow * (x - t_slow))
    hp = x - t_slow
    d = t_fast[..., pa] * hp[..., pb] - hp[..., pa] * t_fast[..., pb]
    flow = torch.stack([(d * wts[:, 0]).clamp(-4, 4).mean(dim=-1), (d * wts[:, 1]).clamp(-4, 4).mean(dim=-1)], dim=-1)
    ftb = flow[..., 0] * sign
    rotation = ftb[:, 0] - ftb[:, 1]
    r = p.gain * rotation
    q = r / (1.0 + r.abs())
    o = torch.stack([1.0 - p.delta * q.clamp(min=0), 1.0 - p.delta * (-q).clamp(min=0)], dim=1)
    return flow, rotation, (p.base * o).clamp(p.drive_min, p.drive_max)


def window(fn, calls):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for k in range(calls):
        fn(k)
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / calls          # microseconds per call


variants = {"kernel, same buffer": lambda k: motion.update(buffers[0]),
            "kernel, rotating": lambda k: motion.update(buffers[k % 8]),
            "torch, same buffer": lambda k: torch_rule(buffers[0]),
            "torch, rotating": lambda k: torch_rule(buffers[k % 8])}
for fn in variants.values():                             # warm-up of every timed shape
    window(fn, args.calls)
times = {name: [] for name in variants}
total = {name: 0.0 for name in variants}
while min(total.values()) < args.seconds * 1e6:           # alternated: a window of each in turn
    for name, fn in variants.items():
        us = window(fn, args.calls)
        times[name].append(us)
        total[name] += us * args.calls

# agreement: both flavours from the same state over a few ticks of new readings
motion.reset()
motion.update(buffers[0])
t_fast.copy_(motion.fast); t_slow.copy_(motion.slow)
for k in (1, 2, 3):
    motion.update(buffers[k])
    flow, rotation, drive = torch_rule(buffers[k])
torch.cuda.synchronize()
agreement = dict(flow=float((motion.flow - flow).abs().max()), rotation=float((motion.rotation - rotation).abs().max()),
                 drive=float((motion.drive - drive).abs().max()), flow_scale=float(motion.flow.abs().max()))
# the torch flavour sums 2070 float32 terms of up to 1 and skips the 2^-16 rounding: 2^-16 of a term plus 1e-5 of summation error
ok = agreement["flow"] < 3e-5 and agreement["rotation"] < 6e-5 and agreement["drive"] < 6e-5 * p.gain

# the control tick the update is part of
eyes = EyeRenderer(sim, fly.name, scene=Scene(checker_size=2.0, ground_rgb=((0, 0, 0), (1, 1, 1))))
omm = buffers[1]
with TurningCPG(sim, fly.name) as cpg:
    def tick(k):
        eyes.render_into(omm)
        motion.update(omm, out=cpg.drive)
        cpg.step(steps)

    for _ in range(3):
        window(tick, 10)
    tick_us = statistics.median(window(tick, 10) for _ in range(7))
    eye_us = statistics.median(window(lambda k: eyes.render_into(omm), 10) for _ in range(7))
    in_tick_us = statistics.median(window(lambda k: (eyes.render_into(omm), motion.update(omm, out=cpg.drive)), 10)
                                   for _ in range(7)) - eye_us

model_bytes = n * 2 * n_omm * 24
result = dict(worlds=n, n_omm=n_omm, n_pairs=n_pairs, model_bytes=model_bytes, calls_per_window=args.calls, agreement=agreement,
              agreement_ok=ok, control_steps=steps, control_tick_us=tick_us, eye_render_us=eye_us, update_after_eyes_us=in_tick_us,
              variants={})
for name, us in times.items():
    med = statistics.median(us)
    rate = model_bytes / (med * 1e-6)
    result["variants"][name] = dict(us=dict(median=med, min=min(us), max=max(us), windows=len(us)), model_tb_per_s=rate / 1e12,
                                    share_of_hbm_peak=rate / HBM_PEAK, share_of_control_tick=med / tick_us)
    print(f"{name:20s}: {med:8.1f} us per call (min {min(us):.1f}, max {max(us):.1f}, {len(us)} windows of {args.calls}) = "
          f"{rate / 1e12:.2f} TB/s of the model's {model_bytes / 1e6:.1f} MB = {100 * rate / HBM_PEAK:.0f} % of the HBM peak; "
          f"{100 * med / tick_us:.2f} % of the control tick")
print(f"control tick (render_into + update + cpg.step({steps})): {tick_us:.1f} us; render_into alone {eye_us:.1f} us; "
      f"update right after the eye kernel adds {in_tick_us:.1f} us")
print(f"kernel against torch: max |difference| flow {agreement['flow']:.2e} (largest |flow| {agreement['flow_scale']:.2e}), rotation "
      f"{agreement['rotation']:.2e}, drive {agreement['drive']:.2e} ({'within' if ok else 'OUTSIDE'} the tolerance)")
print(json.dumps(result))
if args.out is not None:
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(result, indent=1) + "\n")
motion.close()
sys.exit(0 if ok else 1)
