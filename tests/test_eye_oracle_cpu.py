"""The eye renderer's specification in its two flavours (oracle/sensors_oracle.py::render_eye_frames, ``dtype`` float32 / float64),
without a GPU: the float32 default draws the bytes it always drew, the float64 flavour passes the hand-worked answers, the two agree
on every interior pixel (tests/eye_parity.py::interior_mask — the rule tests/test_eye_parity_gpu.py holds the kernel to), and known
answers for what the older tests leave out: a camera that looks up, a camera inside a sphere, a lens of 300 degrees, a capsule seen
end-on."""
import functools
import hashlib

import numpy as np
import pytest

import eye_parity as ep
import sensors_oracle as so

render64 = functools.partial(so.render_eye_frames, dtype=np.float64)
# SHA-256 (first 16 hex digits) of the float32 frames.  Recorded from the specification as it was before it took ``dtype`` and
# ``return_materials``, except the starred ones: relief scenes with rays that meet the relief beyond 210 mm, where the probe step
# is now relative (sensors_oracle.TERRAIN_EPS_REL; in float32 t + 1e-4 == t from 1000 mm on, such a ray stood still for 64 cells and
# took the flat answer).  Pixels that changed, all within a row or two of the horizon: 6 and 18 of the known-answer scenes, 1, 1,
# 8 and 18 of the synthetic ones; each of these frames moved TOWARDS the float64 flavour (e.g. 42 -> 32 and 26 -> 12 differing pixels).
KNOWN_ANSWER_DIGESTS = ("a1ca0fab25a0bf9c", "01cfd3acd54b7751", "f15759357e0ff9b7", "9b3cc89765b1d758", "b91234335a4fb08d",     # [3] * [4] *
                        "6e1383c188157a3e", "a1ca0fab25a0bf9c")
SYNTHETIC_DIGESTS = {(0, 0): "366d4d739d2264d3", (0, 1): "d2b29304ff570d26", (1, 0): "6990c7b82e4d2820", (1, 1): "c608f64f323f5f4a",     # (1, 1) *
                     (2, 0): "d23b3e44ec2c44ed", (2, 1): "ac83c1e2891829bb", (3, 0): "bf570e87f1ca0db4", (3, 1): "f9eb722deff0fd81"}     # (2, 0) * (3, 0) * (3, 1) *
DOWN, UP = np.eye(3), np.diag([1.0, -1.0, -1.0])           # camera axes (columns right, up, back): looking along -z / along +z


def _sha(frame):
    return hashlib.sha256(np.ascontiguousarray(frame).tobytes()).hexdigest()[:16]


@functools.lru_cache(maxsize=None)
def _synthetic(kind, seed):
    """(frame32, materials32, frame64, materials64) of a synthetic scene: rendered once, shared, never written to."""
    args, kw = ep.synthetic_scene(kind, seed)
    out = so.render_eye_frames(*args, **kw, return_materials=True) + so.render_eye_frames(*args, **kw, dtype=np.float64, return_materials=True)
    for a in out:
        a.setflags(write=False)
    return out


def test_the_default_flavour_draws_the_bytes_it_drew():
    """Every call of the two known-answer tests of tests/test_sensors.py: the default (float32) frame has the recorded digest
    (KNOWN_ANSWER_DIGESTS), with and without ``return_materials``; the material image decodes to the frame."""
    for (args, kw), digest in zip(ep.known_answer_scenes(), KNOWN_ANSWER_DIGESTS, strict=True):
        frame = so.render_eye_frames(*args, **kw)
        assert _sha(frame) == digest
        frame2, mat = so.render_eye_frames(*args, **kw, return_materials=True)
        assert np.array_equal(frame, frame2) and mat.shape == frame.shape[:2] and mat.min() >= -1
        assert ((mat == 0) == (frame == np.array(ep.SKY, dtype=np.uint8)).all(axis=-1)).all()


@pytest.mark.parametrize("kind, seed", sorted(SYNTHETIC_DIGESTS))
def test_flavours_agree_on_every_interior_pixel(kind, seed):
    """Terrain kinds 0-3, two seeds each, 54 or 55 capsules and two spheres at 512 x 450 and 157 degrees: the float32 frame has the
    recorded digest (SYNTHETIC_DIGESTS); the float32 and the float64 material images differ on NO interior pixel (a
    float32 ray is 1e-4 of a pixel pitch from the float64 one: it can change a material only where a boundary passes that close
    to a pixel centre, and such a pixel has a differing neighbour).  Measured: 0 to 14 differing pixels a frame (at most 6.1e-5),
    interior share 0.89 to 0.93."""
    frame32, mat32, frame64, mat64 = _synthetic(kind, seed)
    assert _sha(frame32) == SYNTHETIC_DIGESTS[(kind, seed)]
    interior = ep.interior_mask(mat64)
    differ = mat32 != mat64
    print(f"eye specification, terrain {kind} seed {seed}: float32 vs float64 differ in {int(differ.sum())} pixels "
          f"({differ.mean():.2e} of the frame; edge pixels {differ.sum() / max((~interior).sum(), 1):.2e}), interior share {interior.mean():.3f}")
    assert not (differ & interior).any()
    assert ((frame32 != frame64).any(axis=-1) == differ).all()          # the frames differ exactly where the materials do
    assert 0.8 < interior.mean() < 0.97                                  # the rule is not vacuous, and the scene is not empty
    assert differ.mean() < 5e-4
    seen = set(np.unique(mat64).tolist())
    assert {0, 1, 2, 4} <= seen and (3 in seen) == (kind != 0) and seen & {5, 6}


def test_interior_rule():
    mat = np.zeros((5, 6), dtype=np.int64)
    mat[2, 3] = 7
    want = np.ones((5, 6), dtype=bool)
    want[1:4, 2:5] = False
    assert np.array_equal(ep.interior_mask(mat), want)
    assert ep.interior_mask(np.full((3, 3), 2)).all()                    # border pixels take the neighbours that exist
    mat = np.zeros((4, 4), dtype=np.int64)
    mat[0, 0] = 1
    assert (~ep.interior_mask(mat)).sum() == 4


def test_float64_flavour_passes_the_hand_worked_answers():
    ep.check_known_answers(render64)
    ep.check_terrain_and_body_known_answers(render64)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_looking_up_sees_only_sky(dtype):
    """A lens of 120 degrees has its widest ray (the corner: rho = 1.33) 80 degrees from the axis: looking along +z no ray points
    below the horizon, whatever lies below — relief, a sphere, a capsule."""
    assert np.hypot(450 / 512, 1.0) * 60.0 < 90.0
    frame, mat = so.render_eye_frames((0.5, 0.5, 1.0), UP, 512, 450, 120.0, 4.0, 0.0, ep.SKY, ep.GROUND, [(0.5, 0.5, 0.3, 0.25)], [(10, 20, 30)],
                                      terrain=ep.TERRAINS[3], wall_rgb=ep.WALL, capsules=[((0.2, 0.5, 0.5), (0.8, 0.5, 0.5), 0.1)], body_rgb=ep.BODY,
                                      dtype=dtype, return_materials=True)
    assert (mat == 0).all() and (frame == np.array(ep.SKY, dtype=np.uint8)).all()
    # the same camera at 157 degrees does see the ground in its corners and along its left and right edges
    _, mat = so.render_eye_frames((0.5, 0.5, 1.0), UP, 512, 450, 157.0, 4.0, 0.0, ep.SKY, ep.GROUND, dtype=dtype, return_materials=True)
    assert mat[0, 0] in (1, 2) and mat[256, 225] == 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_camera_inside_a_sphere_does_not_see_it(dtype):
    """Spheres are surfaces seen from outside (the nearest POSITIVE root of the entry point): from inside, the frame is the one
    without the sphere; a second sphere outside it is seen as before."""
    outside = [(0.5, 0.5, 1.0, 0.4)]
    args = ((0.5, 0.5, 2.0), DOWN, 512, 450, 157.0, 4.0, 0.0, ep.SKY, ep.GROUND)
    without = so.render_eye_frames(*args, outside, [(10, 20, 30)], dtype=dtype)
    within, mat = so.render_eye_frames(*args, outside + [(0.3, 0.6, 2.2, 1.5)], [(10, 20, 30), (200, 0, 0)], dtype=dtype, return_materials=True)
    assert np.array_equal(within, without) and not (mat == 6).any() and (mat == 5).any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_lens_of_300_degrees_has_black_corners(dtype):
    """Pixels whose polar angle rho * 150 degrees exceeds 180 (rho > 1.2) lie behind the fisheye's full sphere: black, and nothing
    else is; rays between 90 and 180 degrees look up, away from the ground below."""
    H, W = 512, 450
    frame, mat = so.render_eye_frames((0.5, 0.5, 2.0), DOWN, H, W, 300.0, 4.0, 0.0, ep.SKY, ep.GROUND, dtype=dtype, return_materials=True)
    i, j = np.mgrid[0:H, 0:W]
    rho = np.hypot((j + 0.5 - W / 2) * 2 / H, (i + 0.5 - H / 2) * 2 / H)
    clear = np.abs(rho - 1.2) > 1e-4
    assert ((mat == -1) == (rho > 1.2))[clear].all()
    assert ((frame == 0).all(axis=-1) == (mat == -1)).all()
    assert mat[0, 0] == -1 and mat[H - 1, W - 1] == -1 and mat[0, W // 2] == 0 and mat[H // 2, W // 2] in (1, 2)
    assert 0 < (mat == -1).sum() == ep.lens_path(H, W, 300.0)[1] < 0.1 * H * W
    above = (rho > 0.6 + 1e-4) & (rho < 1.2 - 1e-4)                      # beyond 90 degrees: sky
    assert (mat[above] == 0).all() and (mat[rho < 0.6 - 1e-4] > 0).all()
    assert not ep.lens_path(H, W, 300.0)[0] and ep.lens_path(H, W, 157.0) == (True, 0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_capsule_seen_end_on_draws_a_disc(dtype):
    """A capsule along the optical axis, its near end cap's centre at distance d: a disc of angular radius asin(r / d) (the cap's
    tangent cone; the cylinder behind it subtends less)."""
    H, W, fov, r, d = 512, 450, 157.0, 0.2, 1.0
    caps = [((0.5, 0.5, 1.0), (0.5, 0.5, 0.3), r)]
    _, mat = so.render_eye_frames((0.5, 0.5, 2.0), DOWN, H, W, fov, 4.0, 0.0, ep.SKY, ep.GROUND, capsules=caps, body_rgb=ep.BODY,
                                  dtype=dtype, return_materials=True)
    i, j = np.mgrid[0:H, 0:W]
    theta = np.hypot((j + 0.5 - W / 2) * 2 / H, (i + 0.5 - H / 2) * 2 / H) * np.radians(fov / 2)
    edge = np.arcsin(r / d)
    assert np.arctan(r / d) < edge
    clear = np.abs(theta - edge) > 1e-5                                   # a thousandth of a pixel pitch from the rim
    assert ((mat == 4) == (theta < edge))[clear].all()
    r_pix = edge / np.radians(fov / 2) * H / 2
    assert abs((mat == 4).sum() - np.pi * r_pix ** 2) < 0.03 * np.pi * r_pix ** 2


def test_lens_paths_of_the_small_retinas():
    """Which lens takes which path on the small retinas of tests/test_eye_parity_gpu.py (tests/eye_parity.py::LENS_PATHS)."""
    for shape, table in ep.LENS_PATHS.items():
        rows, cols = ep.SMALL_RETINAS[shape]
        assert 40 <= rows * cols <= 100 and (shape[0] * shape[1]) % 16 == 0
        for fov, want in table.items():
            assert ep.lens_path(*shape, fov) == want, (shape, fov)
    assert (48 * 64) % 1024 == 0 and 64 % 16 == 0 and 50 % 16 != 0 and 96 % 16 == 0 and (80 * 96) % 1024 != 0
    assert ep.lens_path(512, 450, 157.0) == (True, 0)
