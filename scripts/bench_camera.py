"""Camera-renderer timing (needs the GPU): ms per render for 4 / 64 / 4096 worlds x 1 camera at 240 x 320 on flat ground and blocks,
ns per ray, and the 4096-world stepping rate with and without a 4-world renderer at the default pacing (one frame per 80 steps).
Device events around warmed-up repetitions; writes profiles/camera_bench.txt (or the path given)."""
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import numpy as np, torch
import flygym_amd.compose as C
from flygym_amd import HIPSimulation, make_model
from flygym_amd.controllers import TripodCPG
from flygym_amd.rendering import HIPBatchRenderer
from flygym_amd.utils.math import Rotation3D

out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "camera_bench.txt"
EYE_NS_PER_RAY = 1.880e6 / (8192 * 175776)      # profiles/r6_eyes_summary.md: 1.880 ms per 8192 eye views x 175776 rays
H, W, N = 240, 320, 4096
lines = [f"camera renderer, {H} x {W}, 1 camera (the default tracking camera), {N}-world batch after settle + 300 CPG steps; "
         f"eye kernel for comparison: {EYE_NS_PER_RAY * 1e3:.3f} ps per ray (profiles/r6_eyes_summary.md)"]


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


for world_cls in ("FlatGroundWorld", "BlocksTerrainWorld"):
    fly, world, cam = make_model()
    if world_cls != "FlatGroundWorld":
        world = getattr(C, world_cls)()
        world.add_fly(fly, (0, 0, 0.8), Rotation3D("quat", (1, 0, 0, 0)))
    sim = HIPSimulation(world, n_worlds=N, device=0)
    sim.set_leg_adhesion_states(fly.name, np.ones((N, 6), dtype=np.float32))
    sim.warmup()
    table = TripodCPG(fly.get_actuated_jointdofs_order("position"), sim.timestep).targets(N, 2500, device=sim.device)
    ids = sim.replay_ids(fly.name)
    for k in range(6):
        sim.step_replay(table, ids, 50 * k, 50)
    for n_sel in (4, 64, 4096):
        worlds = list(range(0, N, N // n_sel))
        r = HIPBatchRenderer(sim, cam, worlds=worlds, camera_res=(H, W), buffer_frames=False)
        out = torch.empty((n_sel, 1, H, W, 3), dtype=torch.uint8, device=sim.device)
        reps = 200 if n_sel <= 64 else 20
        timed(lambda: r.render_into(out), 5)                   # warm-up
        ms = [timed(lambda: r.render_into(out), reps) for _ in range(3)]
        best = min(ms)
        lines.append(f"{world_cls:20s} {n_sel:5d} worlds: {best:.4f} ms per render (three windows of {reps}: {', '.join(f'{m:.4f}' for m in ms)}) "
                     f"= {best * 1e6 / (n_sel * H * W):.3f} ns per ray = {best * 1e6 / (n_sel * H * W) / EYE_NS_PER_RAY:.2f} x the eye kernel's")
        r.close()
    if world_cls == "FlatGroundWorld":
        # stepping rate in 20-step launches, with and without a 4-world renderer asked after every launch (a frame every 80 steps)
        def run(renderer, launches=200):
            def tick(k=[0]):
                sim.step_replay(table, ids, 20 * (k[0] % 100), 20); k[0] += 1
                if renderer is not None:
                    renderer.render_as_needed(sim)
            timed(tick, 20)
            return [N * 20 / (timed(tick, launches) * 1e-3) for _ in range(3)]
        plain = run(None)
        r = HIPBatchRenderer(sim, cam, worlds=[0, 1, 2, 3], camera_res=(H, W), buffer_frames=False)
        with_r = run(r)
        plain2 = run(None)
        lines.append(f"stepping {N} worlds in 20-step launches: {max(plain + plain2) / 1e6:.2f} M env-steps/s without a renderer "
                     f"(windows {', '.join(f'{v / 1e6:.2f}' for v in plain + plain2)}), {max(with_r) / 1e6:.2f} M with a 4-world renderer at the "
                     f"default pacing (windows {', '.join(f'{v / 1e6:.2f}' for v in with_r)})")
        r.close()
    del sim
out_path.parent.mkdir(parents=True, exist_ok=True)
out_path.write_text("\n".join(lines) + "\n")
print("\n".join(lines))
