#!/usr/bin/env python
"""ms per launch of every renderer kernel, for an A/B of two builds of the library: all six nmf_eye_kernel instantiations
(readings only / with frames / sampled, on the flat ground and on a terrain world) and both camera kernels.

    python scripts/bench_render_ab.py            # one JSON line for the library in use (NMF_HIP_LIB or the in-tree build)
    python scripts/bench_render_ab.py --ab parent tree --reps 5     # build/libnmf_parent.so against the tree, interleaved:
                                                                    # one fresh process per repeat, A B A B ..., then a table

The flies stand at their spawn poses (no stepping: only the renderers run).  Each figure is the mean over --calls launches
between two events, after 3 warm-up launches."""
import argparse
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def measure(calls, eye_worlds, cam_worlds):
    import torch
    import flygym_amd.compose as C
    from flygym_amd import HIPSimulation, make_model
    from flygym_amd.rendering import HIPBatchRenderer
    from flygym_amd.utils.math import Rotation3D
    from flygym_amd.vision import EyeRenderer, Scene

    def timed(fn):
        for _ in range(3):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / calls

    scene = Scene(spheres=[(6.0, 4.0, 1.5, 1.0)], sphere_rgb=[(0.9, 0.2, 0.1)])
    upright = Rotation3D("quat", (1, 0, 0, 0))
    out = {}
    for tag, world_cls in (("flat", None), ("relief", "BlocksTerrainWorld")):
        fly, world, cam = make_model()
        if world_cls:
            world = getattr(C, world_cls)()
            world.add_fly(fly, (0.4, 0.1, 0.8), upright)
        sim = HIPSimulation(world, n_worlds=eye_worlds, device=0)
        eyes = EyeRenderer(sim, fly.name, scene)
        out[f"eye_{tag}_readings"] = timed(eyes.render)
        out[f"eye_{tag}_sampled"] = timed(EyeRenderer(sim, fly.name, scene, rays_per_ommatidium=16).render)
        few = HIPSimulation(world, n_worlds=64, device=0)           # (frames: 1.4 MB per fly)
        out[f"eye_{tag}_frames_64"] = timed(EyeRenderer(few, fly.name, scene).render_frames)
        if world_cls:
            out["camera_relief"] = timed(HIPBatchRenderer(sim, cam, worlds=list(range(cam_worlds)), scene=scene, buffer_frames=False).render)
        else:
            out["camera_flat"] = timed(HIPBatchRenderer(sim, cam, worlds=list(range(cam_worlds)), scene=scene, buffer_frames=False).render)
    alice, world, cam_a = make_model(name="alice")
    bob, _, cam_b = make_model(name="bob")
    world.add_fly(bob, (5.0, 1.5, 0.8), upright)
    sim = HIPSimulation(world, n_worlds=cam_worlds, device=0)
    out["camera_two_flies"] = timed(HIPBatchRenderer(sim, [cam_a, cam_b], flies="all", scene=scene, buffer_frames=False).render)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ab", nargs=2, metavar=("A", "B"), help="library names as in scripts/gpu_ab.py: build/libnmf_<name>.so, or `tree`")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--eye-worlds", type=int, default=1024)
    ap.add_argument("--cam-worlds", type=int, default=64)
    a = ap.parse_args()
    if not a.ab:
        print(json.dumps(measure(a.calls, a.eye_worlds, a.cam_worlds)))
        return
    runs = {name: [] for name in a.ab}
    for rep in range(a.reps):
        for name in a.ab:
            env = dict(os.environ)
            env.pop("NMF_HIP_LIB", None)
            if name != "tree":
                env["NMF_HIP_LIB"] = str(ROOT / "build" / f"libnmf_{name}.so")
            r = subprocess.run([sys.executable, __file__, "--calls", str(a.calls), "--eye-worlds", str(a.eye_worlds), "--cam-worlds", str(a.cam_worlds)],
                               env=env, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                sys.exit(f"{name}, repeat {rep}: exit status {r.returncode}\n{r.stderr[-2000:]}")
            runs[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(name, rep, r.stdout.strip().splitlines()[-1], flush=True)
    A, B = a.ab
    print(f"\nms per launch, {a.reps} interleaved repeats ({A} {B} {A} {B} ...); bar: median of {B} <= highest repeat of {A}")
    print(f"{'case':22s} {A + ' min':>10s} {A + ' med':>10s} {A + ' max':>10s}   {B + ' min':>10s} {B + ' med':>10s} {B + ' max':>10s}   bar")
    for case in runs[A][0]:
        va, vb = [r[case] for r in runs[A]], [r[case] for r in runs[B]]
        print(f"{case:22s} {min(va):10.4f} {statistics.median(va):10.4f} {max(va):10.4f}   {min(vb):10.4f} {statistics.median(vb):10.4f} {max(vb):10.4f}   "
              f"{'met' if statistics.median(vb) <= max(va) else 'MISSED'}")


if __name__ == "__main__":
    main()
