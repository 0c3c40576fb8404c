"""Batch camera renderer on the GPU (``flygym_amd/csrc/nmf_camera.hip``, ``flygym_amd/rendering.py``) against its numpy
specification ``tests/camera_spec.py``."""
import ctypes

import numpy as np
import pytest

import camera_spec as cs

pytestmark = pytest.mark.gpu

WORLDS = ["FlatGroundWorld", "GappedTerrainWorld", "BlocksTerrainWorld", "MixedTerrainWorld"]
KEYS = ("qpos", "qvel", "ctrl", "qacc_warmstart", "seg_xpos", "seg_xquat", "site_xpos", "actuator_force", "sensordata", "time",
        "stats", "qacc", "stats_sum", "contact_geom", "act")
SPHERE = (3.0, 2.0, 1.5, 1.0)


@pytest.fixture
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch


def _top_camera():
    from flygym_amd.utils.math import Rotation3D

    return dict(name="topcam", mode="fixed", pos=(0.0, 0.0, 12.0), rotation=Rotation3D("xyaxes", (1, 0, 0, 0, 1, 0)), fovy=45.0)


def _walking(world_cls="FlatGroundWorld", n=64):
    """n worlds of the benchmark fly, settled, with a CPG table whose phase differs from world to world."""
    import flygym_amd.compose as C
    from flygym_amd import HIPSimulation, make_model
    from flygym_amd.controllers import TripodCPG
    from flygym_amd.utils.math import Rotation3D

    fly, world, cam = make_model()
    if world_cls != "FlatGroundWorld":
        world = getattr(C, world_cls)()
        world.add_fly(fly, (0, 0, 0.8), Rotation3D("quat", (1, 0, 0, 0)))
    sim = HIPSimulation(world, n_worlds=n, device=0)
    sim.set_leg_adhesion_states(fly.name, np.ones((n, 6), dtype=np.float32))
    sim.warmup()
    table = TripodCPG(fly.get_actuated_jointdofs_order("position"), sim.timestep).targets(n, 2500, device=sim.device)
    return sim, fly, cam, table, sim.replay_ids(fly.name)


def _id_scene():
    """Colours that name the hit: with ambient 1 and diffuse 0 a frame's red byte is the hit id of the kernel."""
    from flygym_amd.vision import Scene

    u = lambda *c: tuple(v / 255.0 for v in c)
    scene = Scene(sky_rgb=u(1, 2, 3), ground_rgb=(u(10, 0, 0), u(20, 0, 0)), wall_rgb=u(30, 0, 0), spheres=[SPHERE], sphere_rgb=[u(40, 0, 0)])
    cap = np.array([u(100 + k, 1, 1) for k in range(69)])
    return scene, cap


def _kernel_ids(frame):
    r = frame[..., 0].astype(np.int64)
    out = np.full(r.shape, -1, dtype=np.int64)
    for red, hid in ((1, cs.SKY), (10, cs.GROUND_A), (20, cs.GROUND_B), (30, cs.WALL), (40, cs.SPHERE0)):
        out[r == red] = hid
    caps = r >= 100
    out[caps] = cs.CAPSULE0 + r[caps] - 100
    assert (out >= 0).all()
    return out


def _spec_inputs(sim, renderer, w, cam_i):
    """What the specification needs for world w and camera cam_i, from the batch's poses (float64)."""
    from flygym_amd.rendering import camera_pose

    nseg = len(renderer.capsule_seg)
    xpos = sim.field("seg_xpos")[w].cpu().numpy().reshape(-1, 3).astype(np.float64)
    xquat = sim.field("seg_xquat")[w].cpu().numpy().reshape(-1, 4).astype(np.float64)
    assert nseg == 69 == len(xpos)
    mode, pos, mat, fovy = camera_pose(renderer.cameras[cam_i])
    cam_pos = pos + xpos[0] if mode == "track" else pos          # segment 0 is the root
    terrain = None
    if sim.model["terrain_type"][0] != 0:
        tp = sim.model["terrain_params"]
        terrain = (int(sim.model["terrain_type"][0]), tuple(float(v) for v in tp[:4]), float(tp[4]))
    caps = cs.world_capsules(xpos, xquat, renderer.capsule_seg, renderer.capsule_geom)
    sc = renderer.scene
    kw = dict(checker_size=sc.checker_size, ground_z=0.0, sky_rgb=sc.sky_rgb, ground_rgb=sc.ground_rgb, wall_rgb=sc.wall_rgb,
              spheres=[SPHERE], sphere_rgb=sc.sphere_rgb, terrain=terrain, capsules=caps, capsule_rgb=renderer.capsule_rgb,
              ambient=renderer.ambient, diffuse=renderer.diffuse)
    return (cam_pos, mat, renderer.camera_res[0], renderer.camera_res[1], fovy), kw


def _check_parity(sim, fly, cams, torch, worlds, label):
    """Check 1 on the batch's current poses.  Returns (largest spec32-vs-spec64 share, largest kernel-vs-spec64 share, hit ids)."""
    from flygym_amd.rendering import HIPBatchRenderer
    from flygym_amd.vision import Scene

    id_scene, id_caps = _id_scene()
    shaded = HIPBatchRenderer(sim, cams, worlds=worlds, scene=Scene(spheres=[SPHERE], sphere_rgb=[(0.9, 0.2, 0.1)]))
    coded = HIPBatchRenderer(sim, cams, worlds=worlds, scene=id_scene, capsule_rgb=id_caps, ambient=1.0, diffuse=0.0)
    fr, fr_id = shaded.render().cpu().numpy(), coded.render().cpu().numpy()
    assert fr.shape == (len(worlds), len(cams), 240, 320, 3)
    n_pix = 240 * 320
    worst_spec = worst_kernel = 0.0
    all_ids = {}
    for wi, w in enumerate(worlds):
        for ci in range(len(cams)):
            args, kw = _spec_inputs(sim, shaded, w, ci)
            rgb64, hit64 = cs.render(*args, **kw, dtype=np.float64)
            _, hit32 = cs.render(*args, **kw, dtype=np.float32)
            ids = _kernel_ids(fr_id[wi, ci])
            spec_share, kernel_share = float((hit32 != hit64).mean()), float((ids != hit64).mean())
            same = ids == hit64
            err = np.abs(fr[wi, ci].astype(np.int64) - rgb64.astype(np.int64))[same]
            print(f"camera parity {label} world {w} camera {ci}: spec32 vs spec64 {spec_share:.3e}, kernel vs spec64 {kernel_share:.3e}, "
                  f"max grey-level error on equal hits {int(err.max())}")
            worst_spec, worst_kernel = max(worst_spec, spec_share), max(worst_kernel, kernel_share)
            all_ids[(w, ci)] = ids
            assert err.max() <= 1, (label, w, ci, int(err.max()))
    bar = max(4.0 * worst_spec, 2.0 / n_pix)
    print(f"camera parity {label}: largest spec32-vs-spec64 share {worst_spec:.3e}, bar {bar:.3e}, kernel's largest share {worst_kernel:.3e}")
    assert worst_kernel <= bar, (label, worst_kernel, bar)
    shaded.close(); coded.close()
    return worst_spec, worst_kernel, all_ids


@pytest.mark.parametrize("world_cls", WORLDS)
def test_pixel_parity_with_the_specification(torch_mod, world_cls):
    """64 worlds, settle + 200 CPG steps with per-world phases, worlds [41, 3, 17, 60], the default tracking camera and a fixed
    one looking straight down from 12 mm, 240 x 320, one sphere.  Against tests/camera_spec.py in float64 on the same poses:
    (a) the share of pixels whose hit id differs, per image, is at most FOUR TIMES the largest share by which the specification
    in float32 differs from itself in float64 on these poses (never less than 2 pixels of an image); (b) where the hit id
    agrees every channel is within 1 grey level (float32 against float64 shading can cross one rounding boundary, no more).
    The kernel's hit ids are read from a second render with colours that name the hit (ambient 1, diffuse 0).
    Measured (profiles/camera_parity.txt): the specification in float32 differs from itself in float64 in 1.3e-5 ... 1.6e-4 of an image's
    pixels (1 ... 12 pixels), so the bars are 4.2e-4 ... 6.3e-4; the kernel differs from the float64 specification in 0 pixels of every
    image, and its channels are within 1 grey level everywhere."""
    sim, fly, cam, table, ids = _walking(world_cls)
    sim.step_replay(table, ids, 0, 200)
    torch_mod.cuda.synchronize()
    _, _, hit = _check_parity(sim, fly, [cam, _top_camera()], torch_mod, [41, 3, 17, 60], world_cls)
    seen = set(np.unique(np.concatenate([v.ravel() for v in hit.values()])))
    assert cs.SPHERE0 in seen and any(h >= cs.CAPSULE0 for h in seen) and (cs.GROUND_A in seen and cs.GROUND_B in seen)
    if world_cls != "FlatGroundWorld":
        assert cs.WALL in seen


def test_selection_of_worlds_and_cameras(torch_mod):
    """worlds=[5, 2] gives, bit for bit, rows 5 and 2 of a render of all 64 worlds; a list of cameras gives the single-camera
    frames in list order."""
    torch = torch_mod
    from flygym_amd.rendering import HIPBatchRenderer

    sim, fly, cam, table, ids = _walking()
    sim.step_replay(table, ids, 0, 200)
    top = _top_camera()
    res = (120, 160)
    every = HIPBatchRenderer(sim, [cam, top], camera_res=res).render()
    assert every.shape == (64, 2, 120, 160, 3) and every.dtype == torch.uint8 and every.device == sim.device
    two = HIPBatchRenderer(sim, [cam, top], worlds=[5, 2], camera_res=res).render()
    assert torch.equal(two[0], every[5]) and torch.equal(two[1], every[2]) and not torch.equal(every[5], every[2])
    swapped = HIPBatchRenderer(sim, [top, cam], worlds=[5, 2], camera_res=res).render()
    only_cam = HIPBatchRenderer(sim, "trackcam", worlds=[5, 2], camera_res=res).render()
    only_top = HIPBatchRenderer(sim, top, worlds=[5, 2], camera_res=res).render()
    assert torch.equal(swapped[:, 0], two[:, 1]) and torch.equal(swapped[:, 1], two[:, 0])
    assert torch.equal(only_cam[:, 0], two[:, 0]) and torch.equal(only_top[:, 0], two[:, 1])
    # an image size that is no multiple of the tile or of four: the row segments' odd bytes
    odd = HIPBatchRenderer(sim, [cam, top], worlds=[5, 2], camera_res=(37, 43))
    canvas = torch.full((2 * 2 * 37 * 43 * 3 + 64,), 7, dtype=torch.uint8, device=sim.device)
    out = odd.render_into(canvas[:2 * 2 * 37 * 43 * 3].view(2, 2, 37, 43, 3))
    torch.cuda.synchronize()
    assert bool((canvas[2 * 2 * 37 * 43 * 3:] == 7).all())              # nothing written past the frames
    args, kw = _spec_inputs(sim, odd, 2, 0)
    kw.update(spheres=[], sphere_rgb=[])
    rgb, _ = cs.render(args[0], args[1], 37, 43, args[4], **kw)
    assert (np.abs(out[1, 0].cpu().numpy().astype(int) - rgb.astype(int)).max(axis=-1) > 1).mean() < 0.02


def test_tracking_camera_follows_the_fly(torch_mod):
    """After the walk the root has moved by more than a checker square (4 mm); the tracking camera's frame still has capsule hits
    within the centre third of the image, the fixed camera's hits moved; both still pass check 1.

    The walk is 10 000 CPG steps (1 s), not the 2000 first planned: the tripod gait of ``controllers.py`` covers 1.2-1.4 mm in
    2000 steps (measured: 1.37 and 1.23 mm in worlds 41 and 3), so 2000 steps never leave the first checker square.  The
    displacement asked for is unchanged — what the check needs is a fly that has left the place it was filmed at."""
    torch = torch_mod
    from flygym_amd.controllers import TripodCPG

    sim, fly, cam, table, ids = _walking()
    sim.step_replay(table, ids, 0, 200)
    torch.cuda.synchronize()
    cams, worlds = [cam, _top_camera()], [41, 3]
    start = sim.get_body_positions(fly.name)[:, 0].cpu().numpy().copy()
    _, _, before = _check_parity(sim, fly, cams, torch, worlds, "before the walk")
    cpg = TripodCPG(fly.get_actuated_jointdofs_order("position"), sim.timestep)
    for piece in range(4):
        part = cpg.targets(64, 2500, start_step=200 + 2500 * piece, device=sim.device)
        for k in range(50):
            sim.step_replay(part, ids, 50 * k, 50)
        torch.cuda.synchronize()
    moved = np.linalg.norm(sim.get_body_positions(fly.name)[:, 0].cpu().numpy() - start, axis=1)
    print("root displacement after 10000 steps (mm):", moved[worlds])
    assert (moved[worlds] > 4.0).all()
    _, _, after = _check_parity(sim, fly, cams, torch, worlds, "after the walk")
    for w in worlds:
        centre = after[(w, 0)][80:160, 107:213]
        assert (centre >= cs.CAPSULE0).mean() > 0.02            # the tracking camera still looks at the fly
        was, now = before[(w, 1)] >= cs.CAPSULE0, after[(w, 1)] >= cs.CAPSULE0
        assert (was & now).sum() < 0.5 * was.sum()              # the fixed camera's fly walked out of its old silhouette


def test_the_engine_does_not_notice_the_renderer(torch_mod):
    """Two batches from the same seed, one rendering every 20 steps: all state and output fields bitwise equal after 400 steps."""
    torch = torch_mod
    from flygym_amd.rendering import HIPBatchRenderer

    a = _walking("BlocksTerrainWorld")
    b = _walking("BlocksTerrainWorld")
    r = HIPBatchRenderer(b[0], [b[2], _top_camera()], worlds=[0, 63, 7])
    for k in range(20):
        for sim, fly, cam, table, ids in (a, b):
            sim.step_replay(table, ids, 20 * k, 20)
        r.render()
    torch.cuda.synchronize()
    assert len(r.frames) == 20 and not torch.equal(r.frames[0], r.frames[-1])
    for key in KEYS:
        assert torch.equal(a[0].field(key), b[0].field(key)), key


def test_step_and_render_are_one_captured_graph(torch_mod):
    """``step(20)`` + ``nmf_camera_render`` captured with ``torch.cuda.graph`` on the batch's stream (a single chain) replays to
    frames bit-equal to the eager calls: the render call allocates nothing and never synchronises."""
    torch = torch_mod
    from flygym_amd.rendering import HIPBatchRenderer

    sims, rends, outs = [], [], []
    for _ in range(2):
        sim, fly, cam, table, ids = _walking()
        sims.append((sim, table, ids))
        rends.append(HIPBatchRenderer(sim, [cam, _top_camera()], worlds=[9, 1, 30], buffer_frames=False))
        outs.append(torch.zeros((3, 2, 240, 320, 3), dtype=torch.uint8, device=sim.device))
    torch.cuda.synchronize()
    frames = []
    for tick in range(4):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):                      # captured before this renderer has ever rendered
            sims[1][0].step_replay(sims[1][1], sims[1][2], 20 * tick, 20)
            rends[1].render_into(outs[1])
        g.replay()
        torch.cuda.synchronize()
        sims[0][0].step_replay(sims[0][1], sims[0][2], 20 * tick, 20)
        rends[0].render_into(outs[0])
        torch.cuda.synchronize()
        assert torch.equal(outs[0], outs[1]), tick
        for key in KEYS:
            assert torch.equal(sims[0][0].field(key), sims[1][0].field(key)), (tick, key)
        frames.append(outs[0].clone())
    assert not torch.equal(frames[0], frames[-1])          # the flies moved
    assert int(frames[-1].max()) > 0


def test_set_renderer_surface(torch_mod, tmp_path, capsys):
    torch = torch_mod
    from PIL import Image
    from flygym_amd import HIPSimulation, make_model
    from flygym_amd.rendering import HIPBatchRenderer
    from flygym_amd.utils.math import Rotation3D

    sim, fly, cam, table, ids = _walking()
    sim.reset()
    sim.set_leg_adhesion_states(fly.name, np.ones((64, 6), dtype=np.float32))
    # refusals come before anything is launched
    with pytest.raises(NotImplementedError):
        sim.set_renderer(cam, worlds=[0, 1], use_gpu_batch_rendering=False)
    with pytest.raises(RuntimeError):
        sim.set_renderer(cam, worlds=[0, 1], use_gpu_batch_rendering=True, scene_option=object())
    for bad in ([64], [3, 3], [-1]):
        with pytest.raises(ValueError):
            sim.set_renderer(cam, worlds=bad, use_gpu_batch_rendering=True)
    with pytest.raises(ValueError):
        sim.set_renderer("nosuchcam", worlds=[0], use_gpu_batch_rendering=True)
    with pytest.raises(ValueError, match="'fixed' and 'track'"):
        sim.set_renderer(dict(cam, mode="targetbody"), worlds=[0], use_gpu_batch_rendering=True)
    assert sim.renderer is None and sim.render_as_needed() == {}
    # the library's own validation (a binding that skips the Python checks)
    from flygym_amd import _native
    from flygym_amd.rendering import _CameraParams
    good = HIPBatchRenderer(sim, cam, worlds=[0])
    lib = _native.lib()
    for ids_bad in ([64], [1, 1]):
        arr = np.asarray(ids_bad, dtype=np.int32)
        assert not lib.nmf_camera_plan_create(sim._batch_h, ctypes.byref(good._params), 1, arr.ctypes.data, len(arr), None, None, None, 0)
        assert b"world id" in lib.nmf_last_error()
    one = np.zeros(1, dtype=np.int32)
    seg = np.asarray([69], dtype=np.int32); geom = np.ones(7, dtype=np.float32); rgb = np.zeros(3, dtype=np.uint8)
    assert not lib.nmf_camera_plan_create(sim._batch_h, ctypes.byref(good._params), 1, one.ctypes.data, 1, seg.ctypes.data, geom.ctypes.data, rgb.ctypes.data, 1)
    assert not lib.nmf_camera_plan_create(sim._batch_h, ctypes.byref(good._params), 9, one.ctypes.data, 1, None, None, None, 0)
    assert not lib.nmf_camera_plan_create(sim._batch_h, ctypes.byref(good._params), 1, one.ctypes.data, 1, seg.ctypes.data, geom.ctypes.data, rgb.ctypes.data, 73)
    good.close()

    r = sim.set_renderer(cam, worlds=[0, 1], use_gpu_batch_rendering=True)
    assert isinstance(r, HIPBatchRenderer) and sim.renderer is r
    # 400 steps of 0.1 ms, render_as_needed after every 20: calls at 2, 4, ..., 40 ms.  The first call renders; then a frame is
    # due once 8 ms have passed since the last one: 2, 10, 18, 26, 34 ms — calls 0, 4, 8, 12, 16 of the 20
    assert abs(sim.timestep - 1e-4) < 1e-12
    got = []
    for k in range(20):
        sim.step_replay(table, ids, 20 * k, 20)
        got.append(sim.render_as_needed())
    assert [i for i, g in enumerate(got) if g] == [0, 4, 8, 12, 16] and len(r.frames) == 5
    assert r.frames[0].shape == (2, 1, 240, 320, 3)
    r.save_video(1, tmp_path / "world1")
    first = np.array(Image.open(sorted((tmp_path / "world1").glob("*.png"))[0]))
    assert np.array_equal(first, r.frames[0][1, 0].cpu().numpy())
    r.save_video([0, 1], tmp_path / "both.gif")
    with Image.open(tmp_path / "both.gif") as im:
        assert im.n_frames == 5
    # the profiled call fills the report's render time and frame count
    sim.reset()
    assert r.frames == [] and sim._frames_rendered == 0 and sim._total_render_time_ns == 0
    sim.set_leg_adhesion_states(fly.name, np.ones((64, 6), dtype=np.float32))
    for _ in range(3):
        sim.step_with_profile()
        sim.render_as_needed_with_profile()
    assert sim._frames_rendered == 1 and sim._total_render_time_ns > 0
    sim.print_performance_report()
    assert "PERFORMANCE" in capsys.readouterr().out
    with r:
        pass
    with pytest.raises(RuntimeError):
        r.render()

    # a world with two flies: out of scope, and said so
    fly_a, world, cam_a = make_model(name="alice")
    fly_b, _, _ = make_model(name="bob")
    world.add_fly(fly_b, (6.0, 0, 0.8), Rotation3D("quat", (1, 0, 0, 0)))
    both = HIPSimulation(world, n_worlds=2, device=0)
    with pytest.raises(NotImplementedError, match="several flies"):
        both.set_renderer(cam_a, worlds=[0], use_gpu_batch_rendering=True)
