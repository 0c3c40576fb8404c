"""Time ``SensorySteering.update`` on the GPU: 4096 worlds x 2 eyes x 721 ommatidia plus one odor dimension, against the same
rule written with torch operations (several passes with temporaries; it sums floats, so its results are compared within a
tolerance), and against a 20-step control tick with the eye renderer (``render_into`` -> ``update`` -> ``cpg.step(20)``).

The two flavours alternate in the same process after a warm-up; each is timed by device events over windows of --calls calls until
at least --seconds have been measured.  The readings are 47 MB, less than the Infinity Cache: "same buffer" re-reads one tensor
(as the tick does, right after the eye kernel wrote it), "rotating" walks over eight tensors (378 MB) so that every call reads from
HBM.  The traffic model is one read of the readings, n x 2 x n_omm x 8 bytes; its rate is set against the 8 TB/s HBM peak.
Results go to stdout and, as JSON, to --out (recorded by hand in profiles/taxis_summary.md).  Needs an MI355X: no fallback."""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
from flygym_amd import HIPSimulation, make_model
from flygym_amd.controllers import SensorySteering, TurningCPG
from flygym_amd.vision import EyeRenderer, Scene

parser = argparse.ArgumentParser()
parser.add_argument("--worlds", type=int, default=4096)
parser.add_argument("--calls", type=int, default=50)
parser.add_argument("--seconds", type=float, default=0.5)
parser.add_argument("--control-steps", type=int, default=20)
parser.add_argument("--out", type=Path, default=None)
args = parser.parse_args()
if not torch.cuda.is_available():
    sys.exit("taxis_bench.py measures on the GPU and found none")

HBM_PEAK = 8.0e12
n = args.worlds
fly, world, _ = make_model()
sim = HIPSimulation(world, n_worlds=n, device=0)
sim.set_leg_adhesion_states(fly.name, np.ones((n, 6), dtype=np.float32))
sim.warmup()
dev = sim.device
steer = SensorySteering(sim, fly.name, odor_gains=(1.0,))
n_omm, H, W = steer.n_omm, steer.retina.height, steer.retina.width
p = steer._params
rng = np.random.default_rng(0)


def readings():
    r = rng.uniform(0.2, 1.0, (n, 2, n_omm)).astype(np.float32)
    r[rng.random(r.shape) < 0.05] = 0.05
    pale = steer.retina.pale_mask != 0
    return torch.as_tensor(np.stack([np.where(pale, 0, r), np.where(pale, r, 0)], axis=-1).astype(np.float32), device=dev)


buffers = [readings() for _ in range(8)]
odor = torch.as_tensor(rng.uniform(0.0, 2.0, (n, 1, 4)).astype(np.float32), device=dev)
centre = steer.centres.to(torch.float32) / 16.0
front = torch.tensor(steer.front_edge, device=dev, dtype=torch.bool)
gains = steer._gains[:1]


def torch_rule(omm):
    """The same rule in torch operations (float sums; a clamp of the count stands in for the cnt == 0 branch)."""
    dark = (omm[..., 0] + omm[..., 1]) < p.obj_threshold
    cnt = dark.sum(dim=2)
    den = cnt.clamp(min=1).to(torch.float32)
    darkf = dark.to(torch.float32)
    cx = torch.where(cnt > 0, (darkf * centre[:, 0]).sum(dim=2) / (den * W), torch.full_like(den, 0.5))
    cy = torch.where(cnt > 0, (darkf * centre[:, 1]).sum(dim=2) / (den * H), torch.full_like(den, 0.5))
    area = cnt.to(torch.float32) / n_omm
    feat = torch.stack([cy, cx, area], dim=-1)
    devn = torch.where(front, 1.0 - cx, cx)
    v = torch.where(area > p.area_threshold, (1.0 - p.visual_gain * devn).clamp(p.v_min, p.v_max), torch.ones_like(cx))
    L = p.w_ant * odor[..., 2] + p.w_palp * odor[..., 0]
    R = p.w_ant * odor[..., 3] + p.w_palp * odor[..., 1]
    s = L + R
    c = torch.where(s > 0, (L - R) / s.clamp(min=1e-30), torch.zeros_like(s))
    b = (gains * c).sum(dim=1)
    q = b * b.abs() / (1.0 + b * b)
    o = torch.stack([1.0 - p.odor_delta * q.clamp(min=0), 1.0 - p.odor_delta * (-q).clamp(min=0)], dim=1)
    return feat, b, (p.base * v * o).clamp(p.drive_min, p.drive_max)


def window(fn, calls):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for k in range(calls):
        fn(k)
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / calls          # microseconds per call


variants = {"kernel, same buffer": lambda k: steer.update(omm=buffers[0], odor=odor),
            "kernel, rotating": lambda k: steer.update(omm=buffers[k % 8], odor=odor),
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

steer.update(omm=buffers[3], odor=odor)
feat, b, d = torch_rule(buffers[3])
torch.cuda.synchronize()
agreement = dict(features=float((steer.features - feat).abs().max()), bias=float((steer.bias - b).abs().max()),
                 drive=float((steer.drive - d).abs().max()))
# the torch flavour sums 721 floats of up to 512 in float32 and divides with the library's fast division: 1e-4 of the image
ok = agreement["features"] < 1e-4 and agreement["bias"] < 1e-5 and agreement["drive"] < 1e-3

# the control tick the update is part of
steps = args.control_steps
eyes = EyeRenderer(sim, fly.name, scene=Scene(spheres=[(8.0, 4.0, 1.3, 2.0)], sphere_rgb=[(0.0, 0.0, 0.0)]))
omm = buffers[1]
with TurningCPG(sim, fly.name) as cpg:
    def tick(k):
        eyes.render_into(omm)
        steer.update(omm=omm, odor=odor, out=cpg.drive)
        cpg.step(steps)

    for _ in range(3):
        window(tick, 10)
    tick_us = statistics.median(window(tick, 10) for _ in range(7))
    eye_us = statistics.median(window(lambda k: eyes.render_into(omm), 10) for _ in range(7))
    in_tick_us = statistics.median(window(lambda k: (eyes.render_into(omm), steer.update(omm=omm, odor=odor, out=cpg.drive)), 10)
                                   for _ in range(7)) - eye_us

model_bytes = n * 2 * n_omm * 8
result = dict(worlds=n, n_omm=n_omm, model_bytes=model_bytes, calls_per_window=args.calls, agreement=agreement, agreement_ok=ok,
              control_steps=steps, control_tick_us=tick_us, eye_render_us=eye_us, update_after_eyes_us=in_tick_us, variants={})
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
print(f"kernel against torch: max |difference| features {agreement['features']:.2e}, bias {agreement['bias']:.2e}, "
      f"drive {agreement['drive']:.2e} ({'within' if ok else 'OUTSIDE'} the tolerance)")
print(json.dumps(result))
if args.out is not None:
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(result, indent=1) + "\n")
sys.exit(0 if ok else 1)
