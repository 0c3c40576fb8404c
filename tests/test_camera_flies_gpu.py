"""Batch camera renderer for worlds with several flies (``set_renderer(..., flies=...)``; ``nmf_camera_flies_kernel`` of
``flygym_amd/csrc/nmf_camera.hip``) against the numpy specification ``tests/camera_spec.py`` with the capsules of the drawn
flies concatenated in fly order.  Small shapes: 4 worlds, worlds [3, 1] selected, 70 x 101 images (neither side a multiple of
the 32-pixel tile, the width no multiple of 4)."""
import ctypes

import numpy as np
import pytest

import camera_spec as cs
from test_camera_gpu import KEYS, _kernel_ids

pytestmark = pytest.mark.gpu

N, WORLDS, RES = 4, [3, 1], (70, 101)
SPHERE = (3.0, 2.0, 1.5, 1.0)
LOOK_X = np.array([[0.0, 0, -1.0], [-1.0, 0, 0], [0, 1.0, 0]])          # right = -y, up = +z, back = -x: looks along +x


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch


def _top_camera(x=3.0):
    from flygym_amd.utils.math import Rotation3D

    return dict(name="topcam", mode="fixed", pos=(x, 0.0, 12.0), rotation=Rotation3D("xyaxes", (1, 0, 0, 0, 1, 0)), fovy=45.0)


def _two_flies(bob_at=(6.0, 0.0, 0.8), bob_yaw_deg=45.0, steps=100, same_inputs=False):
    """4 worlds with alice at the origin and bob at ``bob_at``, settled, then ``steps`` CPG steps — bob half a second further
    into the gait than alice unless ``same_inputs``."""
    from flygym_amd import HIPSimulation, make_model
    from flygym_amd.controllers import TripodCPG
    from flygym_amd.utils.math import Rotation3D

    alice, world, cam_a = make_model(name="alice")
    bob, _, cam_b = make_model(name="bob")
    half = np.deg2rad(bob_yaw_deg) / 2
    world.add_fly(bob, bob_at, Rotation3D("quat", (float(np.cos(half)), 0.0, 0.0, float(np.sin(half)))))
    sim = HIPSimulation(world, n_worlds=N, device=0)
    tables = {}
    for k, (name, fly) in enumerate(world.fly_lookup.items()):
        sim.set_leg_adhesion_states(name, np.ones((N, 6), dtype=np.float32))
        cpg = TripodCPG(fly.get_actuated_jointdofs_order("position"), sim.timestep)
        tables[name] = (cpg.targets(N, 400, start_step=0 if same_inputs else 5000 * k, device=sim.device), sim.replay_ids(name))
    sim.warmup()

    def walk(start, count):
        for name, (table, ids) in tables.items():
            sim.for_fly(name).step_replay(table, ids, start, count)

    if steps:
        walk(0, steps)
    return sim, (cam_a, cam_b), walk


@pytest.fixture(scope="module")
def walked(torch_mod):
    """The two-fly batch of checks 1, 2, 4 and 5 after its 100 steps; these tests only read it."""
    sim, cams, _ = _two_flies()
    torch_mod.cuda.synchronize()
    return sim, cams


def _id_scene(n_flies):
    """Colours that name the hit: with ambient 1 and diffuse 0 a frame's red byte is the kernel's hit id — capsule k of fly f
    is 100 + 69 f + k."""
    from flygym_amd.vision import Scene

    u = lambda *c: tuple(v / 255.0 for v in c)
    scene = Scene(sky_rgb=u(1, 2, 3), ground_rgb=(u(10, 0, 0), u(20, 0, 0)), wall_rgb=u(30, 0, 0), spheres=[SPHERE], sphere_rgb=[u(40, 0, 0)])
    return scene, [np.array([u(100 + 69 * f + k, 1, 1) for k in range(69)]) for f in range(n_flies)]


def _renderers(sim, cams, flies="all"):
    """(shaded, id-coded) renderers of the same cameras."""
    from flygym_amd.rendering import HIPBatchRenderer
    from flygym_amd.vision import Scene

    shaded = HIPBatchRenderer(sim, cams, worlds=WORLDS, camera_res=RES, flies=flies, scene=Scene(spheres=[SPHERE], sphere_rgb=[(0.9, 0.2, 0.1)]))
    scene, caps = _id_scene(len(shaded.fly_names))
    coded = HIPBatchRenderer(sim, cams, worlds=WORLDS, camera_res=RES, flies=flies, scene=scene, ambient=1.0, diffuse=0.0,
                             capsule_rgb=dict(zip(shaded.fly_names, caps)))
    return shaded, coded


def _spec_inputs(sim, rend, w, cam_i):
    """What the specification needs for world w and camera cam_i: the drawn flies' capsules concatenated in fly order."""
    from flygym_amd.rendering import camera_pose

    poses = {}
    for name in rend.fly_names:
        b = sim.for_fly(name)
        poses[name] = (b.field("seg_xpos")[w].cpu().numpy().reshape(-1, 3).astype(np.float64),
                       b.field("seg_xquat")[w].cpu().numpy().reshape(-1, 4).astype(np.float64))
    mode, pos, mat, fovy = camera_pose(rend.cameras[cam_i])
    owner = rend.enabled_cam_names[cam_i].split("/")[0]
    cam_pos = pos + poses[owner][0][rend._params.cam[cam_i].track_seg] if mode == "track" else pos
    caps, rgb = [], []
    for name in rend.fly_names:
        caps += cs.world_capsules(*poses[name], rend.capsule_seg[name], rend.capsule_geom[name])
        rgb += list(rend.capsule_rgb[name])
    sc = rend.scene
    kw = dict(checker_size=sc.checker_size, ground_z=0.0, sky_rgb=sc.sky_rgb, ground_rgb=sc.ground_rgb, wall_rgb=sc.wall_rgb,
              spheres=[SPHERE], sphere_rgb=sc.sphere_rgb, capsules=caps, capsule_rgb=rgb, ambient=rend.ambient, diffuse=rend.diffuse)
    return (cam_pos, mat, RES[0], RES[1], fovy), kw


def _check_parity(sim, cams, label):
    """The bars of the single-fly test (tests/test_camera_gpu.py) on the batch's current poses: per image, the share of pixels
    whose hit id differs from the float64 specification is at most four times the largest share by which the specification in
    float32 differs from itself in float64 on these poses, never less than 2 pixels; where the ids agree every channel is
    within 1 grey level.  Returns the kernel's hit ids by (world, camera)."""
    shaded, coded = _renderers(sim, cams)
    fr, fr_id = shaded.render().cpu().numpy(), coded.render().cpu().numpy()
    assert fr.shape == (len(WORLDS), len(cams), *RES, 3)
    n_pix = RES[0] * RES[1]
    worst_spec = worst_kernel = 0.0
    all_ids = {}
    for wi, w in enumerate(WORLDS):
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
    return all_ids


BOB0 = cs.CAPSULE0 + 69          # the first hit id of bob's capsules


def test_pixel_parity_with_the_specification(walked):
    """Alice's tracking camera, bob's, and a fixed camera straight down from 12 mm above x = 3, one sphere in the scene.
    Measured (profiles/camera_flies.txt): the specification in float32 differs from itself in float64 in 0 or 1 of an image's
    7070 pixels, so the bar is 4 pixels; the kernel differs from the float64 specification in 0 pixels of every image."""
    sim, (cam_a, cam_b) = walked
    ids = _check_parity(sim, [cam_a, cam_b, _top_camera()], "two flies")
    for w in WORLDS:
        top = ids[(w, 2)]
        assert ((top >= cs.CAPSULE0) & (top < BOB0)).any() and (top >= BOB0).any()          # both flies under the fixed camera
        assert (ids[(w, 1)][23:47, 34:67] >= BOB0).mean() > 0.02                             # bob's camera shows bob
        mine = ids[(w, 0)][23:47, 34:67]
        assert ((mine >= cs.CAPSULE0) & (mine < BOB0)).mean() > 0.02                         # and alice's shows alice
    assert any((v == cs.SPHERE0).any() for v in ids.values())


def test_occlusion(walked):
    """A fixed camera on the line through both thoraxes (world 3's), 5 mm behind alice, looking along +x: bob stands behind
    alice and is partly hidden."""
    sim, _ = walked
    a = sim.get_body_positions("alice")[3, 0].cpu().numpy().astype(np.float64)
    b = sim.get_body_positions("bob")[3, 0].cpu().numpy().astype(np.float64)
    u = (b - a) / np.linalg.norm(b - a)
    assert u[0] > 0.99                                        # the line through the thoraxes runs along +x
    cam = dict(name="behind", mode="fixed", pos=tuple(a - 5.0 * u), rotation=LOOK_X, fovy=40.0)
    ids = _check_parity(sim, [cam], "occlusion")
    for w in WORLDS:
        frame = ids[(w, 0)]
        assert ((frame >= cs.CAPSULE0) & (frame < BOB0)).any() and (frame >= BOB0).any()
    # partly hidden: without alice more pixels show bob
    shaded, coded = _renderers(sim, [cam], flies=["bob"])
    alone = _kernel_ids(coded.render().cpu().numpy()[0, 0])          # (one drawn fly: its capsules are ids CAPSULE0 ...)
    assert (alone >= cs.CAPSULE0).sum() > (ids[(3, 0)] >= BOB0).sum() > 0
    shaded.close(); coded.close()


def test_tie_rule(torch_mod):
    """Two flies of the same model at the same spawn pose with the same inputs: their poses are bit-equal, every capsule pixel
    is hit twice at the same distance, and the earlier fly wins each of them."""
    torch = torch_mod
    sim, (cam_a, _), _ = _two_flies(bob_at=(0.0, 0.0, 0.8), bob_yaw_deg=0.0, steps=40, same_inputs=True)
    torch.cuda.synchronize()
    for key in ("seg_xpos", "seg_xquat"):
        assert torch.equal(sim.for_fly("alice").field(key), sim.for_fly("bob").field(key)), key
    cams = [cam_a, _top_camera(0.0)]
    shaded, coded = _renderers(sim, cams)
    red = coded.render()[..., 0]
    assert bool(((red >= 100) & (red < 169)).any()) and not bool((red >= 169).any())
    shaded_one, coded_one = _renderers(sim, cams, flies=["alice"])
    assert torch.equal(coded.frames[0], coded_one.render()) and torch.equal(shaded.render(), shaded_one.render())
    for r in (shaded, coded, shaded_one, coded_one):
        r.close()


def test_selection_of_flies(walked, torch_mod):
    """flies=["alice"] is, bit for bit, the single-fly renderer of alice's batch; a list's order does not matter."""
    torch = torch_mod
    from flygym_amd.rendering import HIPBatchRenderer
    from flygym_amd.vision import Scene

    sim, (cam_a, cam_b) = walked
    scene = Scene(spheres=[SPHERE], sphere_rgb=[(0.9, 0.2, 0.1)])
    kw = dict(worlds=WORLDS, camera_res=RES, scene=scene, buffer_frames=False)
    cams = [cam_a, _top_camera()]
    with HIPBatchRenderer(sim, cams, flies=["alice"], **kw) as one, HIPBatchRenderer(sim.for_fly("alice"), cams, **kw) as single:
        assert one.enabled_cam_names == single.enabled_cam_names == ["alice/trackcam", "alice/topcam"]
        assert list(one.capsule_seg) == ["alice"] and np.array_equal(one.capsule_seg["alice"], single.capsule_seg)
        frames = one.render()
        assert torch.equal(frames, single.render()) and int(frames.max()) > 0
    cams = [cam_a, cam_b, _top_camera()]
    with HIPBatchRenderer(sim, cams, flies="all", **kw) as every, HIPBatchRenderer(sim, cams, flies=["bob", "alice"], **kw) as listed:
        assert every.fly_names == listed.fly_names == ["alice", "bob"]
        assert every.enabled_cam_names == ["alice/trackcam", "bob/trackcam", "alice/topcam"]
        both = every.render()
        assert torch.equal(both, listed.render())
        assert not torch.equal(both[:, 2], frames[:, 1])          # bob is in the fixed camera's image


def test_refusals_before_any_launch(walked):
    from flygym_amd import HIPSimulation, _native, make_model
    from flygym_amd.rendering import HIPBatchRenderer, _CameraFly

    sim, (cam_a, cam_b) = walked
    on = dict(worlds=WORLDS, use_gpu_batch_rendering=True)
    for bad in (["carol"], ["alice", "alice"], []):
        with pytest.raises(ValueError):
            sim.set_renderer(cam_a, flies=bad, **on)
    with pytest.raises(ValueError, match="tracks fly 'bob'"):
        sim.set_renderer([cam_a, cam_b], flies=["alice"], **on)
    with pytest.raises(ValueError, match="at most 8"):
        sim.set_renderer([_top_camera()] * 9, flies="all", **on)
    with pytest.raises(NotImplementedError, match=r"several flies.*flies="):
        sim.set_renderer(cam_a, **on)
    with pytest.raises(NotImplementedError):
        sim.set_renderer(cam_a, worlds=WORLDS, flies="all", use_gpu_batch_rendering=False)
    with pytest.raises(RuntimeError):
        sim.set_renderer(cam_a, flies="all", scene_option=object(), **on)
    with pytest.raises(ValueError):
        sim.set_renderer(None, flies="all", **on)
    with pytest.raises(ValueError, match="several flies"):
        HIPBatchRenderer(sim.for_fly("alice"), cam_a, flies="all")
    assert sim.renderer is None and sim.render_as_needed() == {}

    # the library's own validation (a binding that skips the Python checks)
    lib = _native.lib()
    good = HIPBatchRenderer(sim, [cam_a, cam_b], worlds=WORLDS, camera_res=RES, flies="all")
    params, ids, cam_fly = ctypes.byref(good._params), np.asarray(WORLDS, dtype=np.int32), np.asarray([0, 1], dtype=np.int32)
    handles = [sim.for_fly(n)._batch_h for n in ("alice", "bob")]

    def records(batches):
        rec = (_CameraFly * len(batches))()
        for r, h in zip(rec, batches):
            r.batch, r.n_caps = h, 0
        return rec

    def refused(rec, n_flies, cam_fly, text):
        assert not lib.nmf_camera_plan_create_flies(rec, n_flies, params, cam_fly.ctypes.data, 2, ids.ctypes.data, len(ids))
        assert text in lib.nmf_last_error(), lib.nmf_last_error()

    plan = lib.nmf_camera_plan_create_flies(records(handles), 2, params, cam_fly.ctypes.data, 2, ids.ctypes.data, len(ids))
    assert plan
    lib.nmf_camera_plan_destroy(plan)
    refused(records([handles[0], None]), 2, cam_fly, b"batch of fly 1 is null")
    refused(records(handles), 2, np.asarray([0, 2], dtype=np.int32), b"cam_fly[1] = 2")
    refused(records(handles), 2, np.asarray([-1, 0], dtype=np.int32), b"cam_fly[0] = -1")
    refused(records(handles * 3), 5, cam_fly, b"NMF_CAMERA_MAX_FLIES")
    _, lone_world, _ = make_model(name="carol")
    lone = HIPSimulation(lone_world, n_worlds=2, device=0)
    refused(records([handles[0], lone._batch_h]), 2, cam_fly, b"has 2 worlds, fly 0's has 4")
    # a plan of several flies is not the single-fly entry's, and the other way round
    assert lib.nmf_camera_render(handles[0], good._plan_h, None, None, None) != 0 and b"several flies" in lib.nmf_last_error()
    with HIPBatchRenderer(sim.for_fly("alice"), cam_a, worlds=WORLDS, camera_res=RES) as single:
        assert lib.nmf_camera_render_flies(single._plan_h, None, None, None) != 0 and b"one fly" in lib.nmf_last_error()
    good.close()


def test_the_engine_does_not_notice_the_renderer(torch_mod):
    """Two simulations from the same start, one rendering after every 20 steps: every field of both flies' batches is bitwise
    equal after 200 steps."""
    torch = torch_mod
    from flygym_amd.rendering import HIPBatchRenderer

    a, b = _two_flies(steps=0), _two_flies(steps=0)
    r = HIPBatchRenderer(b[0], [*b[1], _top_camera()], worlds=WORLDS, camera_res=RES, flies="all")
    for k in range(10):
        a[2](20 * k, 20); b[2](20 * k, 20)
        r.render()
    torch.cuda.synchronize()
    assert len(r.frames) == 10 and not torch.equal(r.frames[0], r.frames[-1])
    for name in ("alice", "bob"):
        for key in KEYS:
            assert torch.equal(a[0].for_fly(name).field(key), b[0].for_fly(name).field(key)), (name, key)
    r.close()


def test_render_into_is_one_captured_node(torch_mod):
    """``render_into`` a caller's tensor captured with ``torch.cuda.graph`` on its own: the graph is a single chain (here one
    kernel node, no edges), and a replay after further eager steps gives the eager ``render()`` of those poses."""
    torch = torch_mod
    from flygym_amd import _native
    from flygym_amd.rendering import HIPBatchRenderer

    sim, cams, walk = _two_flies(steps=40)
    r = HIPBatchRenderer(sim, [*cams, _top_camera()], worlds=WORLDS, camera_res=RES, flies="all", buffer_frames=False)
    out = torch.zeros((len(WORLDS), 3, *RES, 3), dtype=torch.uint8, device=sim.device)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g):                          # captured before this renderer has ever rendered
        r.render_into(out)
    hip, graph = _native.lib(), ctypes.c_void_p(g.raw_cuda_graph())
    n_nodes, n_edges = ctypes.c_size_t(0), ctypes.c_size_t(0)
    hip.hipGraphGetNodes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    hip.hipGraphGetEdges.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    assert hip.hipGraphGetNodes(graph, None, ctypes.byref(n_nodes)) == 0 and hip.hipGraphGetEdges(graph, None, None, ctypes.byref(n_edges)) == 0
    assert n_nodes.value == 1 and n_edges.value == 0          # a chain of n nodes has n - 1 edges: no parallel branches
    g.replay()
    torch.cuda.synchronize()
    first = out.clone()
    assert torch.equal(first, r.render())
    walk(40, 60)                                       # eager steps; the graph knows nothing of them
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, r.render()) and not torch.equal(out, first)
    r.close()


def test_set_renderer_surface(torch_mod, tmp_path, capsys):
    torch = torch_mod
    from PIL import Image
    from flygym_amd.rendering import HIPBatchRenderer

    sim, (cam_a, cam_b), walk = _two_flies(steps=0)
    sim.reset()
    for name in ("alice", "bob"):
        sim.set_leg_adhesion_states(name, np.ones((N, 6), dtype=np.float32))
    r = sim.set_renderer([cam_a, cam_b], worlds=WORLDS, camera_res=RES, use_gpu_batch_rendering=True, flies="all")
    assert isinstance(r, HIPBatchRenderer) and sim.renderer is r and r.fly_names == ["alice", "bob"]
    # 400 steps of 0.1 ms, render_as_needed after every 20: calls at 2, 4, ..., 40 ms.  The first call renders; then a frame is
    # due once 8 ms have passed since the last one: 2, 10, 18, 26, 34 ms — calls 0, 4, 8, 12, 16 of the 20
    assert abs(sim.timestep - 1e-4) < 1e-12
    got = []
    for k in range(20):
        walk(20 * k, 20)
        got.append(sim.render_as_needed())
    assert [i for i, g in enumerate(got) if g] == [0, 4, 8, 12, 16] and len(r.frames) == 5
    assert r.frames[0].shape == (2, 2, *RES, 3)
    r.save_video(1, {"bob/trackcam": tmp_path / "world1"})
    first = np.array(Image.open(sorted((tmp_path / "world1").glob("*.png"))[0]))
    assert np.array_equal(first, r.frames[0][1, 1].cpu().numpy())
    # reset clears frames and pacing; the profiled call fills the report's render time and frame count
    sim.reset()
    assert r.frames == [] and sim._frames_rendered == 0 and sim._total_render_time_ns == 0
    for name in ("alice", "bob"):
        sim.set_leg_adhesion_states(name, np.ones((N, 6), dtype=np.float32))
    for _ in range(3):
        sim.step_with_profile()
        sim.render_as_needed_with_profile()
    assert sim._frames_rendered == 1 and sim._total_render_time_ns > 0 and len(r.frames) == 1
    sim.print_performance_report()
    assert "PERFORMANCE" in capsys.readouterr().out
    with r:
        pass
    with pytest.raises(RuntimeError):
        r.render()
