"""Batch camera renderer, the parts that need no GPU: the specification (tests/camera_spec.py) against closed forms, the
camera conventions, pacing, files, and the C ABI's layout."""
import ctypes

import numpy as np
import pytest

import camera_spec as cs

GROUND = ((77, 77, 77), (102, 102, 102))
DOWN = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]])        # right = +x, up = +y, back = +z: looks straight down


def test_spec_camera_above_the_origin_sees_the_checker_formula():
    H, W, fovy, z, s = 48, 64, 40.0, 12.0, 4.0
    rgb, hit = cs.render((0.3, -0.2, z), DOWN, H, W, fovy, checker_size=s, ground_rgb=GROUND)
    t = np.tan(np.deg2rad(fovy) / 2) / (H / 2)
    for row in range(H):
        for col in range(W):
            # pixel -> ground point: x = cam_x + z u, y = cam_y - z v (y up in the image is +y in the world)
            x, y = 0.3 + z * (col + 0.5 - W / 2) * t, -0.2 - z * (row + 0.5 - H / 2) * t
            par = (int(np.floor(x / s)) + int(np.floor(y / s))) & 1
            assert hit[row, col] == cs.GROUND_A + par
            assert tuple(rgb[row, col]) == GROUND[par]            # ambient + diffuse = 1 on a surface that faces the light


@pytest.mark.parametrize("axis", ["vertical", "horizontal"])
def test_spec_capsule_under_the_light(axis):
    H, W, fovy, z, r = 240, 320, 30.0, 12.0, 0.5
    base = (120, 90, 60)
    caps = [((0, 0, 1.0), (0, 0, 3.0), r)] if axis == "vertical" else [((-2.0, 0, 2.0), (2.0, 0, 2.0), r)]
    amb, dif = 0.3, 0.5
    # camera on the z axis looking down; the image centre lies between four pixels, so look at the pixel next to it
    rgb, hit = cs.render((0, 0, z), DOWN, H, W, fovy, capsules=caps, capsule_rgb=[base], ambient=amb, diffuse=dif)
    c = rgb[H // 2, W // 2].astype(float)
    want = np.array(base) * (amb + dif)
    assert hit[H // 2, W // 2] == cs.CAPSULE0 and np.all(np.abs(c - want) <= 1.0)      # n_z = 1 to within a pixel's slope
    # silhouette width across the axis: 2 r (H/2) / (tan(fovy/2) distance) to within one pixel
    top = 3.0 + r if axis == "vertical" else 2.0          # the widest cross-section: vertical = the cylinder seen end-on at its top cap's equator
    if axis == "vertical":
        dist = z - 3.0                                    # the equator of the upper end sphere
        width = (hit[H // 2] == cs.CAPSULE0).sum()
    else:
        dist = z - 2.0                                    # the axis
        width = (hit[:, W // 2] == cs.CAPSULE0).sum()
    want_w = 2 * r * (H / 2) / (np.tan(np.deg2rad(fovy) / 2) * dist)
    # (perspective: the tangent cone touches the sphere / cylinder slightly above the equator: a factor 1 / sqrt(1 - (r/dist)^2) < 1.002)
    assert abs(width - want_w) <= 1.0, (width, want_w, top)


def test_spec_side_wall_is_ambient_only():
    # blocks terrain (kind 2): cells of 1.5 mm, odd cells raised by 1 mm.  A camera low over a low cell looking along +x sees
    # the side wall of the next (raised) cell
    terrain = (2, (1.5, 1.0, 0.0, 0.0), 1.0)
    look_x = np.array([[0.0, 0, -1.0], [-1.0, 0, 0], [0, 1.0, 0]])          # right = -y, up = +z, back = -x
    assert np.allclose(look_x.T @ look_x, np.eye(3)) and np.isclose(np.linalg.det(look_x), 1.0)
    amb = 0.35
    rgb, hit = cs.render((0.75, 0.75, 0.5), look_x, 32, 32, 20.0, terrain=terrain, wall_rgb=(60, 40, 20), ambient=amb, diffuse=0.6)
    # (the relief is followed by downward rays only, as for the eyes: the lower half of this image)
    mid = hit[17:28, 8:24]
    assert np.all(mid == cs.WALL)
    assert np.all(rgb[17:28, 8:24] == np.floor(np.array((60, 40, 20)) * amb + 0.5).astype(np.uint8))
    # from above, the raised cell's top faces the light: the checker colours unshaded at ambient + diffuse = 1
    rgb2, hit2 = cs.render((2.25, 0.75, 6.0), DOWN, 32, 32, 5.0, terrain=terrain, ambient=0.4, diffuse=0.6)
    assert set(np.unique(hit2)) <= {cs.GROUND_A, cs.GROUND_B} and tuple(rgb2[16, 16]) in GROUND


def test_default_tracking_camera_geometry():
    from flygym_amd.compose.fly import Fly
    from flygym_amd.rendering import camera_pose

    import inspect
    sig = inspect.signature(Fly.add_tracking_camera)
    cam = dict(name="trackcam", mode=sig.parameters["mode"].default, pos=sig.parameters["pos_offset"].default,
               rotation=sig.parameters["rotation"].default, fovy=sig.parameters["fovy"].default)
    mode, off, mat, fovy = camera_pose(cam)
    assert mode == "track" and fovy == 30.0 and tuple(off) == (0.0, -7.5, 6.0)
    assert np.allclose(mat, [[1, 0, 0], [0, 0.6, -0.8], [0, 0.8, 0.6]])
    # the image centre's ray: camera-frame (0, 0, -1) -> world (0, 0.8, -0.6)
    centre = mat @ np.array([0.0, 0.0, -1.0])
    assert np.allclose(centre, (0, 0.8, -0.6))
    # it meets the horizontal plane through the root segment 0.5 mm ahead of the root in y
    root = np.array([3.0, -2.0, 1.1])
    t = -off[2] / centre[2]
    assert np.allclose(root + off + t * centre, root + (0, 0.5, 0))
    # the rays of an even-sized image straddle the centre symmetrically
    rays = cs.pixel_rays(4, 6, 30.0)
    assert np.allclose(rays[1:3, 2:4].mean(axis=(0, 1))[:2], 0) and np.allclose(np.linalg.norm(rays, axis=-1), 1)
    tpx = np.tan(np.deg2rad(15.0)) / 2
    assert np.allclose(rays[0, 0] / -rays[0, 0, 2], (-2.5 * tpx, 1.5 * tpx, -1))


@pytest.mark.parametrize("fmt,values", [("quat", (0.5, 0.5, -0.5, 0.5)), ("quat", (2.0, 0, 0, 1.0)), ("axisangle", (1, 2, 3, 0.7)),
                                        ("xyaxes", (1, 0, 0, 0, 0.6, 0.8)), ("xyaxes", (1, 1, 0, 0, 1, 1)), ("zaxis", (0.2, -0.3, 0.9)),
                                        ("zaxis", (0, 0, -1)), ("zaxis", (0, 0, 2)), ("euler", (0.3, -1.1, 2.0))])
def test_every_rotation_format_gives_a_rotation_matrix(fmt, values):
    from flygym_amd.utils.math import Rotation3D

    R = Rotation3D(fmt, values).as_matrix()
    assert R.shape == (3, 3) and np.allclose(R.T @ R, np.eye(3), atol=1e-12) and np.isclose(np.linalg.det(R), 1.0)
    if fmt == "xyaxes":
        x = np.array(values[:3], dtype=float); x /= np.linalg.norm(x)
        assert np.allclose(R[:, 0], x) and R[:, 1] @ np.array(values[3:]) > 0 and np.allclose(R[:, 2], np.cross(R[:, 0], R[:, 1]))
    if fmt == "zaxis":
        assert np.allclose(R[:, 2], np.array(values) / np.linalg.norm(values))
    if fmt == "euler":        # extrinsic x, y, z: the z rotation is applied last
        cz, sz = np.cos(values[2]), np.sin(values[2])
        Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
        Rxy = Rotation3D("euler", (values[0], values[1], 0.0)).as_matrix()
        assert np.allclose(R, Rz @ Rxy)
    if fmt in ("quat", "axisangle"):
        w, x, y, z = Rotation3D(fmt, values).as_quat()
        axis = np.array([x, y, z])
        if np.linalg.norm(axis) > 0:
            assert np.allclose(R @ axis, axis)           # the rotation axis stays


def test_unsupported_camera_mode_is_refused_by_name():
    from flygym_amd.rendering import camera_pose

    with pytest.raises(ValueError, match="'fixed' and 'track'"):
        camera_pose(dict(name="c", mode="targetbody", pos=(0, 0, 1), fovy=30.0))


def test_pacing_a_frame_every_8_ms_and_on_the_first_call():
    from flygym_amd.rendering import _Pacer

    p = _Pacer(playback_speed=0.2, output_fps=25)
    assert np.isclose(p.secs_between_renders, 0.008)
    dt = 1e-4
    due = [k for k in range(0, 401) if p.due(k * dt)]
    assert due == [0, 80, 160, 240, 320, 400]
    p.reset()
    # called after every 20 steps from step 20 on: first call, then whenever 8 ms have passed since the last frame
    assert [k for k in range(20, 401, 20) if p.due(k * dt)] == [20, 100, 180, 260, 340]
    p.reset()
    assert p.due(123.0) and not p.due(123.0079) and p.due(123.0081)


def _synthetic_buffer(n_frames=5, worlds=(4, 9, 2), res=(12, 16)):
    from flygym_amd.rendering import _FrameBuffer

    rng = np.random.default_rng(3)
    buf = _FrameBuffer(list(worlds), ["fly/trackcam"], res, output_fps=25)
    for _ in range(n_frames):
        buf._frames.append(rng.integers(0, 256, (len(worlds), 1, *res, 3), dtype=np.uint8))
    return buf


def test_save_video_round_trips_through_pillow(tmp_path):
    from PIL import Image

    buf = _synthetic_buffer()
    want = [f[1, 0] for f in buf.frames]                 # world 9 is row 1 of the selection
    buf.save_video(9, tmp_path / "frames")               # no suffix: a directory of numbered PNGs
    files = sorted((tmp_path / "frames").glob("*.png"))
    assert len(files) == 5
    for f, w in zip(files, want):
        assert np.array_equal(np.array(Image.open(f)), w)
    buf.save_video(9, tmp_path / "clip.png")             # APNG: lossless
    with Image.open(tmp_path / "clip.png") as im:
        assert im.n_frames == 5
        for i, w in enumerate(want):
            im.seek(i)
            assert np.array_equal(np.array(im.convert("RGB")), w)
    buf.save_video(9, tmp_path / "clip.gif")
    with Image.open(tmp_path / "clip.gif") as im:
        assert im.n_frames == 5 and im.info["duration"] == 40          # 25 frames per second
    with pytest.raises(ValueError):
        buf.save_video(5, tmp_path / "other.gif")        # a world that was not rendered


def test_other_containers_need_imageio_and_say_so(tmp_path):
    buf = _synthetic_buffer()
    try:
        import imageio  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match=r"\.gif.*\.png.*\.webp"):
            buf.save_video(4, tmp_path / "clip.mp4")
    # (with imageio installed the mp4 path is imageio's: nothing of this project's to check)


def test_multi_world_grid_has_the_reference_rows_and_columns():
    from flygym_amd.rendering import grid_shape

    # reference warp/rendering.py:219-221: rows = ceil(sqrt(n)), columns = ceil(n / rows)
    assert [grid_shape(n) for n in (1, 2, 3, 4, 5, 6, 7, 9, 10)] == [(1, 1), (2, 1), (2, 2), (2, 2), (3, 2), (3, 2), (3, 3), (3, 3), (4, 3)]
    buf = _synthetic_buffer(n_frames=2, worlds=(4, 9, 2), res=(24, 32))
    merged = buf._fetch_frames_to_cpu_multipleworlds([2, 4, 9], 0, scale=1.0)
    assert len(merged) == 2 and merged[0].shape == (2 * 24, 2 * 32, 3)
    assert not merged[0][24:, 32:].any()                 # the fourth cell of the 2 x 2 grid stays black
    # a cell is that world's frame except where its label was drawn
    cell = merged[1][0:24, 32:64]
    assert (cell == buf.frames[1][0, 0]).mean() > 0.7    # world 4: second in the list -> row 0, column 1
    default = buf._fetch_frames_to_cpu_multipleworlds([2, 4, 9], 0, None)      # scale 1 / columns
    assert default[0].shape == (2 * 12, 2 * 16, 3)


def test_camera_abi():
    from flygym_amd import _native
    from flygym_amd.rendering import _CameraParams

    lib = _native.lib()
    assert lib.nmf_camera_params_size() == ctypes.sizeof(_CameraParams)
    for name in ("nmf_camera_plan_create", "nmf_camera_plan_destroy", "nmf_camera_render"):
        assert hasattr(lib, name) and name in _native.exported_symbols()
