"""Cost of compositing several flies in the camera renderer (needs the GPU): one 240 x 320 frame of 64 selected worlds of a
two-fly world, through (a) the single-fly renderer of alice's batch, (b) the several-flies path with alice drawn, (c) the same
with both flies drawn.  HIP events around every launch, warm-up first, the median of 30 launches; the three cases take turns.
Also the kernels' register / LDS / spill figures (scripts/kernel_stats.py).  Prints, and writes the path given (default
profiles/camera_flies_bench.txt)."""
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import numpy as np
import torch

from flygym_amd import HIPSimulation, make_model
from flygym_amd.controllers import TripodCPG
from flygym_amd.rendering import HIPBatchRenderer
from flygym_amd.utils.math import Rotation3D

out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "camera_flies_bench.txt"
H, W, N, REPS = 240, 320, 64, 30

alice, world, cam_a = make_model(name="alice")
bob, _, _ = make_model(name="bob")
world.add_fly(bob, (6.0, 0, 0.8), Rotation3D("quat", (0.9238795, 0, 0, 0.3826834)))
sim = HIPSimulation(world, n_worlds=N, device=0)
for k, (name, fly) in enumerate(world.fly_lookup.items()):
    sim.set_leg_adhesion_states(name, np.ones((N, 6), dtype=np.float32))
sim.warmup()
for k, (name, fly) in enumerate(world.fly_lookup.items()):
    table = TripodCPG(fly.get_actuated_jointdofs_order("position"), sim.timestep).targets(N, 300, start_step=5000 * k, device=sim.device)
    sim.for_fly(name).step_replay(table, sim.replay_ids(name), 0, 300)
torch.cuda.synchronize()
top = dict(name="topcam", mode="fixed", pos=(3.0, 0.0, 12.0), rotation=Rotation3D("xyaxes", (1, 0, 0, 0, 1, 0)), fovy=45.0)

lines = [f"camera renderer, {H} x {W}, {N} of {N} worlds selected, 1 camera, two-fly world (alice at the origin, bob at x = 6 mm) after settle + "
         f"300 CPG steps; ms per frame, median of {REPS} launches timed one by one with HIP events (the three cases take turns)"]
for label, cam in (("fixed camera 12 mm above x = 3 (both flies in view)", top), ("alice's tracking camera", cam_a)):
    kw = dict(camera_res=(H, W), buffer_frames=False)
    cases = {"single-fly renderer, alice's batch": HIPBatchRenderer(sim.for_fly("alice"), cam, **kw),
             "flies=['alice']": HIPBatchRenderer(sim, cam, flies=["alice"], **kw),
             "flies='all' (alice, bob)": HIPBatchRenderer(sim, cam, flies="all", **kw)}
    out = torch.empty((N, 1, H, W, 3), dtype=torch.uint8, device=sim.device)
    times = {k: [] for k in cases}
    frames = {}
    for rep in range(5 + REPS):
        for name, r in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); r.render_into(out); e1.record(); torch.cuda.synchronize()
            if rep >= 5:
                times[name].append(e0.elapsed_time(e1))
            frames[name] = out.clone()
    med = {k: float(np.median(v)) for k, v in times.items()}
    base = med["single-fly renderer, alice's batch"]
    lines.append(label + ":")
    for name, v in times.items():
        lines.append(f"  {name:36s} {med[name]:.4f} ms (min {min(v):.4f}, max {max(v):.4f}) = {med[name] / base:.3f} x the single-fly renderer")
    same = torch.equal(frames["single-fly renderer, alice's batch"], frames["flies=['alice']"])
    lines.append(f"  flies=['alice'] frames equal the single-fly renderer's bit for bit: {same}")
    for r in cases.values():
        r.close()
stats = subprocess.run([sys.executable, str(ROOT / "scripts" / "kernel_stats.py")], capture_output=True, text=True).stdout
lines += ["kernel figures (scripts/kernel_stats.py):"] + ["  " + " ".join(l.split()) for l in stats.splitlines() if "nmf_camera" in l]
out_path.parent.mkdir(parents=True, exist_ok=True)
out_path.write_text("\n".join(lines) + "\n")
print("\n".join(lines))
