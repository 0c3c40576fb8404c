"""Records tests/golden/render_bits.npz: poses and SHA-256 digests of what the two renderers draw from them.

Run on an MI355X against a build of the commit whose frames are the reference (NMF_HIP_LIB=<its libnmf_hip.so>):

    NMF_HIP_LIB=build/libnmf_parent.so python tests/golden/make_render_bits.py

The poses (seg_xpos / seg_xquat of 2 worlds per world class) are those after the 250-step tumble of
tests/test_sensors.py::test_eye_renderer_sees_the_simulated_world.  tests/test_render_bits_gpu.py writes them back into the
batch and does not step, so the digests depend on the renderers only.  `render_digests` is the one definition of the cases;
the test calls it too.  The digests are never re-recorded from the code under test — with one exception on record: the eye digests of
the gapped, blocks and mixed worlds are those of the build that made the relief walk's probe step relative beyond 210 mm (a fix of
the drawing itself, checked against the float64 specification by tests/test_eye_parity_gpu.py; frames of the build before it differ
in 2 to 38 pixels each, all within 15 rows of the horizon)."""
from __future__ import annotations

import hashlib
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
WORLDS = ("FlatGroundWorld", "GappedTerrainWorld", "BlocksTerrainWorld", "MixedTerrainWorld")
N_WORLDS = 2
CAMERA_RES = (50, 70)         # a width that is no multiple of 4


def make_sim(world_cls):
    import flygym_amd.compose as C
    from flygym_amd import HIPSimulation, make_model
    from flygym_amd.utils.math import Rotation3D

    fly, world, cam = make_model()
    if world_cls != "FlatGroundWorld":
        world = getattr(C, world_cls)()
        world.add_fly(fly, (0.4, 0.1, 0.8), Rotation3D("quat", (1, 0, 0, 0)))
    return HIPSimulation(world, n_worlds=N_WORLDS, device=0), fly, cam


def tumble(sim, fly):
    import torch

    sim.field("qvel")[:, :6] = torch.as_tensor(np.random.default_rng(7).normal(0, 15, (N_WORLDS, 6)), dtype=torch.float32, device=sim.device)
    sim.set_leg_adhesion_states(fly.name, np.ones((N_WORLDS, 6), dtype=np.float32))
    sim.step(250)
    torch.cuda.synchronize()
    return sim.field("seg_xpos").cpu().numpy().copy(), sim.field("seg_xquat").cpu().numpy().copy()


def _sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()


def render_digests(sim, fly, cam, xpos, xquat):
    """{case: digest} of the eye frames, readings, sampled readings and camera frames drawn from the given poses."""
    import torch
    from flygym_amd.rendering import HIPBatchRenderer
    from flygym_amd.utils.math import Rotation3D
    from flygym_amd.vision import EyeRenderer, Scene

    sim.field("seg_xpos").copy_(torch.as_tensor(xpos, device=sim.device).reshape(sim.field("seg_xpos").shape))
    sim.field("seg_xquat").copy_(torch.as_tensor(xquat, device=sim.device).reshape(sim.field("seg_xquat").shape))
    scene = Scene(spheres=[(6.0, 4.0, 1.5, 1.0), (-3.0, 5.0, 2.0, 0.7)], sphere_rgb=[(0.9, 0.2, 0.1), (0.1, 0.8, 0.3)])
    spheres = np.tile(np.asarray(scene.spheres, dtype=np.float32), (N_WORLDS, 1, 1))
    spheres[1, 1, :3] += (1.5, -2.0, 0.5)          # one sphere moved in world 1
    out = {}
    eyes = EyeRenderer(sim, fly.name, scene)
    eyes.set_spheres(spheres)
    frames, omm = eyes.render_frames(with_readings=True)
    out["eye_frames"], out["eye_readings"] = _sha(frames), _sha(omm)
    sampled = EyeRenderer(sim, fly.name, scene, rays_per_ommatidium=16)
    sampled.set_spheres(spheres)
    out["eye_sampled"] = _sha(sampled.render())
    fixed = dict(name="fixedcam", mode="fixed", pos=(2.0, -9.0, 5.0), rotation=Rotation3D("xyaxes", (1, 0, 0, 0, 0.6, 0.8)), fovy=50.0)
    r = HIPBatchRenderer(sim, [fixed, cam], camera_res=CAMERA_RES, scene=scene)
    r.set_spheres(spheres[1])            # (the camera's spheres are shared by all worlds: the moved set)
    out["camera_frames"] = _sha(r.render())
    torch.cuda.synchronize()
    return out


BOB_SHIFT = (5.0, 1.5, 0.0)     # the second fly: the first one's poses, moved by this (mm)


def make_two_fly_sim(world_cls):
    import flygym_amd.compose as C
    from flygym_amd import HIPSimulation, make_model
    from flygym_amd.utils.math import Rotation3D

    alice, world, cam_a = make_model(name="alice")
    bob, _, cam_b = make_model(name="bob")
    upright = Rotation3D("quat", (1, 0, 0, 0))
    if world_cls != "FlatGroundWorld":
        world = getattr(C, world_cls)()
        world.add_fly(alice, (0.4, 0.1, 0.8), upright)
    world.add_fly(bob, (0.4 + BOB_SHIFT[0], 0.1 + BOB_SHIFT[1], 0.8), upright)
    return HIPSimulation(world, n_worlds=N_WORLDS, device=0), (cam_a, cam_b)


def two_fly_digests(sim, cams, xpos, xquat):
    """{case: digest} of the several-flies camera path: both flies drawn, a fixed camera and each fly's track camera."""
    import torch
    from flygym_amd.rendering import HIPBatchRenderer
    from flygym_amd.utils.math import Rotation3D
    from flygym_amd.vision import Scene

    for name, shift in (("alice", (0.0, 0.0, 0.0)), ("bob", BOB_SHIFT)):
        b = sim.for_fly(name)
        pos = np.asarray(xpos, dtype=np.float32).reshape(N_WORLDS, -1, 3) + np.asarray(shift, dtype=np.float32)
        b.field("seg_xpos").copy_(torch.as_tensor(pos, device=b.device).reshape(b.field("seg_xpos").shape))
        b.field("seg_xquat").copy_(torch.as_tensor(xquat, device=b.device).reshape(b.field("seg_xquat").shape))
    scene = Scene(spheres=[(6.0, 4.0, 1.5, 1.0), (-1.5, 3.0, 2.5, 0.7)], sphere_rgb=[(0.9, 0.2, 0.1), (0.1, 0.8, 0.3)])
    fixed = dict(name="fixedcam", mode="fixed", pos=(2.0, -9.0, 5.0), rotation=Rotation3D("xyaxes", (1, 0, 0, 0, 0.6, 0.8)), fovy=50.0)
    r = HIPBatchRenderer(sim, [fixed, *cams], camera_res=CAMERA_RES, flies="all", scene=scene)
    out = {"camera_frames_two_flies": _sha(r.render())}
    torch.cuda.synchronize()
    return out


def main():
    sys.path.insert(0, str(ROOT))
    rec = {}
    for wc in WORLDS:
        sim, fly, cam = make_sim(wc)
        xpos, xquat = tumble(sim, fly)
        rec[f"{wc}/seg_xpos"], rec[f"{wc}/seg_xquat"] = xpos, xquat
        digests = render_digests(sim, fly, cam, xpos, xquat)
        sim2, cams2 = make_two_fly_sim(wc)
        digests.update(two_fly_digests(sim2, cams2, xpos, xquat))
        for case, digest in digests.items():
            rec[f"{wc}/{case}"] = np.array(digest)
            print(wc, case, digest)
    np.savez_compressed(Path(__file__).with_name("render_bits.npz"), **rec)


if __name__ == "__main__":
    main()
