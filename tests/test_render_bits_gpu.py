"""The eye renderer and the batch camera renderer draw, bit for bit, what the commit before nmf_scene.h drew: SHA-256 digests of
frames and readings from fixed poses (tests/golden/render_bits.npz, recorded by tests/golden/make_render_bits.py from a build
of that commit).  The share-of-pixels bounds of test_sensors.py / test_camera_gpu.py would let a refactor move edge pixels;
this does not.  Equality with the recorded digests and nothing else.  (The eye digests of the three relief worlds were
re-recorded once since, when the relief walk's probe step became relative beyond 210 mm — nmf_scene.h kTerrainEpsRel, a float32 stall
of rays that meet the relief a metre away, found by tests/test_eye_parity_gpu.py: 2 to 38 pixels a frame changed, all within 15 rows of
the horizon; the flat world's and every camera digest are the first recording's.)  Per world class: eye frames and readings (own body, two
spheres, one moved in world 1), sampled-mode readings, one-fly camera frames at 50 x 70 from a fixed and a track camera, and
two-fly camera frames of the same size (the second fly: the same poses moved by a constant)."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

GOLDEN = Path(__file__).parent / "golden"
_spec = importlib.util.spec_from_file_location("make_render_bits", GOLDEN / "make_render_bits.py")
mrb = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mrb)


@pytest.mark.gpu
@pytest.mark.parametrize("world_cls", mrb.WORLDS)
def test_renderers_draw_the_recorded_bits(world_cls):
    rec = np.load(GOLDEN / "render_bits.npz")
    sim, fly, cam = mrb.make_sim(world_cls)
    got = mrb.render_digests(sim, fly, cam, rec[f"{world_cls}/seg_xpos"], rec[f"{world_cls}/seg_xquat"])
    sim2, cams2 = mrb.make_two_fly_sim(world_cls)
    got.update(mrb.two_fly_digests(sim2, cams2, rec[f"{world_cls}/seg_xpos"], rec[f"{world_cls}/seg_xquat"]))
    assert set(got) == {"eye_frames", "eye_readings", "eye_sampled", "camera_frames", "camera_frames_two_flies"}
    for case, digest in got.items():
        print(world_cls, case, digest)
    differing = [case for case, digest in got.items() if digest != str(rec[f"{world_cls}/{case}"])]
    assert not differing, f"{world_cls}: {differing} differ from the recorded frames"
