"""Camera renderer for worlds with several flies, the parts that need no GPU: the C ABI's new entry points and the pure
merging of flies, cameras and colours (``flygym_amd.rendering.merge_flies``)."""
import ctypes
import re

import numpy as np
import pytest


def _two_fly_world():
    from flygym_amd import make_model
    from flygym_amd.utils.math import Rotation3D

    alice, world, cam_a = make_model(name="alice")
    bob, _, cam_b = make_model(name="bob")
    world.add_fly(bob, (6.0, 0, 0.8), Rotation3D("quat", (1, 0, 0, 0)))
    return world, cam_a, cam_b


def _top_camera():
    from flygym_amd.utils.math import Rotation3D

    return dict(name="topcam", mode="fixed", pos=(3.0, 0.0, 12.0), rotation=Rotation3D("xyaxes", (1, 0, 0, 0, 1, 0)), fovy=45.0)


def test_the_new_entry_points_are_exported_and_declared():
    from flygym_amd import _native
    from flygym_amd.rendering import MAX_CAMERAS, MAX_FLIES, _CameraParams

    lib = _native.lib()
    header = (_native.INCLUDE / "nmf.h").read_text()
    for name in ("nmf_camera_plan_create_flies", "nmf_camera_render_flies"):
        assert hasattr(lib, name) and name in _native.exported_symbols()
    assert "typedef struct nmf_camera_fly" in header
    limit = int(re.search(r"#define\s+NMF_CAMERA_MAX_FLIES\s+(\d+)", header).group(1))
    assert limit >= 4 and limit == MAX_FLIES
    assert int(re.search(r"#define\s+NMF_CAMERA_MAX\s+(\d+)", header).group(1)) == MAX_CAMERAS
    # the single-fly structure did not move
    assert lib.nmf_camera_params_size() == ctypes.sizeof(_CameraParams)


def test_null_arguments_are_refused_with_a_text():
    from flygym_amd import _native
    from flygym_amd.rendering import _CameraFly, _CameraParams

    lib = _native.lib()
    p, one, ids = _CameraParams(), (_CameraFly * 1)(), np.zeros(1, dtype=np.int32)
    assert not lib.nmf_camera_plan_create_flies(None, 1, ctypes.byref(p), ids.ctypes.data, 1, ids.ctypes.data, 1)
    assert b"nmf_camera_plan_create_flies" in lib.nmf_last_error() and b"null" in lib.nmf_last_error()
    assert not lib.nmf_camera_plan_create_flies(one, 1, None, ids.ctypes.data, 1, ids.ctypes.data, 1)
    assert b"null" in lib.nmf_last_error()
    assert not lib.nmf_camera_plan_create_flies(one, 1, ctypes.byref(p), ids.ctypes.data, 1, ids.ctypes.data, 1)      # a record without a batch
    assert b"batch of fly 0 is null" in lib.nmf_last_error()
    for n in (0, 99):
        assert not lib.nmf_camera_plan_create_flies(one, n, ctypes.byref(p), ids.ctypes.data, 1, ids.ctypes.data, 1)
        assert b"NMF_CAMERA_MAX_FLIES" in lib.nmf_last_error()
    assert lib.nmf_camera_render_flies(None, None, None, None) != 0
    assert b"nmf_camera_render_flies: null plan" in lib.nmf_last_error()


def test_select_flies_orders_and_refusals():
    from flygym_amd.rendering import MAX_FLIES, select_flies

    world, _, _ = _two_fly_world()
    assert list(world.fly_lookup) == ["alice", "bob"]
    assert select_flies(world, "all") == ["alice", "bob"]
    assert select_flies(world, ["bob", "alice"]) == ["alice", "bob"]          # the world's order, not the list's
    assert select_flies(world, ("bob",)) == ["bob"] and select_flies(world, "bob") == ["bob"]
    for bad in (["carol"], ["alice", "alice"], [], ["alice", "bob", "bob"]):
        with pytest.raises(ValueError):
            select_flies(world, bad)

    class Crowd:
        fly_lookup = {f"fly{i}": None for i in range(MAX_FLIES + 1)}

    with pytest.raises(ValueError, match="at most"):
        select_flies(Crowd, "all")
    assert len(select_flies(Crowd, [f"fly{i}" for i in range(MAX_FLIES)])) == MAX_FLIES


def test_merge_flies_arrays_indices_and_defaults():
    from flygym_amd.rendering import merge_flies, resolve_cameras
    from flygym_amd.vision import Scene, body_capsules

    world, cam_a, cam_b = _two_fly_world()
    top = _top_camera()
    resolved = resolve_cameras(world, [cam_b, top, "alice/trackcam"])
    assert [f.name for f, _ in resolved] == ["bob", "alice", "alice"]          # an unowned fixed camera goes to the first fly
    m = merge_flies(world, resolved, "all")
    assert m.fly_names == ["alice", "bob"] and m.cam_fly == [1, 0, 0]
    root = [s.name for s in world.fly_lookup["bob"].get_bodysegs_order()].index(world.fly_lookup["bob"].root_segment.name)
    assert m.track_seg == [root, 0, root]
    seg, geom = body_capsules(world.fly_lookup["alice"], hidden=())
    body = np.asarray(Scene().body_rgb, dtype=np.uint8)
    for name in ("alice", "bob"):
        assert np.array_equal(m.capsule_seg[name], seg) and np.array_equal(m.capsule_geom[name], geom)
        assert m.capsule_seg[name].dtype == np.int32 and m.capsule_geom[name].dtype == np.float32
        assert m.capsule_rgb[name].dtype == np.uint8 and m.capsule_rgb[name].shape == (len(seg), 3)
        assert (m.capsule_rgb[name] == body).all()                            # the default colour
    # colours for one fly only: the other keeps the scene's; rounding as floor(255 x + 0.5)
    k = len(seg)
    colours = np.linspace(0.0, 1.0, 3 * k).reshape(k, 3)
    m2 = merge_flies(world, resolved, ["bob", "alice"], Scene(body_rgb=(9 / 255, 8 / 255, 7 / 255)), {"bob": colours})
    assert m2.fly_names == ["alice", "bob"]
    assert np.array_equal(m2.capsule_rgb["bob"], np.floor(colours * 255.0 + 0.5).astype(np.uint8))
    assert (m2.capsule_rgb["alice"] == np.array([9, 8, 7], dtype=np.uint8)).all()
    # one drawn fly: a fixed camera that belongs to the other one is still welcome, and indices count drawn flies
    m3 = merge_flies(world, resolve_cameras(world, [cam_b, top]), ["bob"])
    assert m3.fly_names == ["bob"] and m3.cam_fly == [0, 0] and list(m3.capsule_seg) == ["bob"]
    # a scene without the body draws no capsules
    m4 = merge_flies(world, resolved, "all", Scene(own_body=False))
    assert all(len(m4.capsule_seg[n]) == 0 and m4.capsule_geom[n].shape == (0, 7) and m4.capsule_rgb[n].shape == (0, 3) for n in m4.fly_names)


def test_merge_flies_refusals():
    from flygym_amd.rendering import MAX_CAMERAS, merge_flies, resolve_cameras

    world, cam_a, cam_b = _two_fly_world()
    top = _top_camera()
    both = resolve_cameras(world, [cam_a, cam_b])
    for bad in (["carol"], ["alice", "alice"], []):
        with pytest.raises(ValueError):
            merge_flies(world, both, bad)
    with pytest.raises(ValueError, match="tracks fly 'bob'"):
        merge_flies(world, both, ["alice"])
    with pytest.raises(ValueError, match="at most"):
        merge_flies(world, resolve_cameras(world, [top] * (MAX_CAMERAS + 1)), "all")
    assert len(merge_flies(world, resolve_cameras(world, [top] * MAX_CAMERAS), "all").cam_fly) == MAX_CAMERAS
    with pytest.raises(ValueError, match="'fixed' and 'track'"):
        merge_flies(world, resolve_cameras(world, [dict(top, mode="targetbody")]), "all")
    k = len(merge_flies(world, both, "all").capsule_seg["alice"])
    with pytest.raises(ValueError, match="dict"):
        merge_flies(world, both, "all", None, np.zeros((k, 3)))
    with pytest.raises(ValueError, match="carol"):
        merge_flies(world, both, "all", None, {"carol": np.zeros((k, 3))})
    with pytest.raises(ValueError, match="one colour per capsule"):
        merge_flies(world, both, "all", None, {"bob": np.zeros((k - 1, 3))})
    with pytest.raises(ValueError, match="not among the drawn"):
        merge_flies(world, resolve_cameras(world, [cam_a]), ["alice"], None, {"bob": np.zeros((k, 3))})
