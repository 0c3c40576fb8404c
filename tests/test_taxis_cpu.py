"""The sensory-steering specification (``tests/taxis_spec.py``) against what it promises — no GPU.

Frames come from the eye renderer's numpy specification (``oracle/sensors_oracle.py``): the two eye cameras at (0.3, +-0.38, 1.3) mm
with the ``EYE_CAMERAS`` orientations over flat ground, a black sphere in view.  Rendered once, shared and read-only."""
import functools

import numpy as np
import pytest

import sensors_oracle as so
import taxis_spec as spec

f32 = np.float32
AZIMUTHS = (30.0, 70.0, -30.0, -70.0)       # degrees from forward, positive to the left


@functools.lru_cache(maxsize=None)
def _retina():
    from flygym_amd.sensors import Retina

    return Retina()


@functools.lru_cache(maxsize=None)
def _table():
    t = _retina().centre_table()
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def _readings(azimuth=None, radius=2.0, distance=8.0):
    """(2, 721, 2) float32 readings of both eyes; the sphere's centre at eye height, ``distance`` mm from the point between the
    cameras.  ``azimuth=None``: no sphere."""
    from flygym_amd.sensors import EYE_CAMERAS, FOVY_PER_EYE_DEG

    r = _retina()
    spheres, rgb = (), ()
    if azimuth is not None:
        a = np.deg2rad(azimuth)
        spheres, rgb = ((0.3 + distance * np.cos(a), distance * np.sin(a), 1.3, radius),), ((0, 0, 0),)
    out = []
    for side, (_, (_, euler)) in zip((+1, -1), EYE_CAMERAS.items()):
        frame = so.render_eye_frames((0.3, side * 0.38, 1.3), so.euler_xyz_extrinsic_to_mat(euler), r.height, r.width, FOVY_PER_EYE_DEG,
                                     4.0, 0.0, (140, 179, 230), ((77, 77, 77), (102, 102, 102)), spheres=spheres, sphere_rgb=rgb)
        out.append(so.retina_resample(frame, r.id_map, r.pale_mask, r.inv_norm))
    out = np.stack(out)
    out.setflags(write=False)
    return out


def _features(*args, **kw):
    r = _retina()
    return spec.features(_readings(*args, **kw), _table(), r.height, r.width)


def test_centres_lie_inside_the_image_and_their_table_fits_int16():
    r = _retina()
    c = r.ommatidia_centres()
    assert c.shape == (721, 2) and c.dtype == np.float64
    assert (c > 0).all() and (c[:, 0] < r.width).all() and (c[:, 1] < r.height).all()
    assert np.allclose(c, spec.ommatidia_centres(r.id_map), rtol=0, atol=1e-9)
    wide = np.rint(16.0 * c)
    assert wide.min() >= 0 and wide.max() <= 32767
    t = r.centre_table()
    assert t.dtype == np.int16 and np.array_equal(t, wide) and np.array_equal(t, spec.centre_table(c))
    assert t[:, 0].astype(np.int64).sum() == 2_595_600 and t[:, 1].astype(np.int64).sum() == 2_953_216
    assert np.abs(t / 16.0 - c).max() <= 1.0 / 32.0


def test_retinas_the_table_cannot_hold_are_refused():
    from flygym_amd.sensors import Retina

    with pytest.raises(ValueError, match="2047"):
        Retina(id_map=np.ones((4, 2048), dtype=np.int16)).centre_table()
    ids = np.arange(1, 1026, dtype=np.int16).reshape(25, 41)
    with pytest.raises(ValueError, match="1024"):
        Retina(id_map=ids).centre_table()
    assert Retina(id_map=np.arange(1, 1025, dtype=np.int16).reshape(32, 32)).centre_table().shape == (1024, 2)


def test_the_frontal_edge_follows_from_the_camera_matrices():
    from flygym_amd.controllers import eye_front_edges
    from flygym_amd.sensors import EYE_CAMERAS

    right_axes = [so.euler_xyz_extrinsic_to_mat(e)[0, 0] for _, (_, e) in EYE_CAMERAS.items()]
    assert right_axes[0] == pytest.approx(0.892, abs=1e-3) and right_axes[1] == pytest.approx(-0.892, abs=1e-3)
    assert spec.front_edge(EYE_CAMERAS) == (1, 0) == eye_front_edges()


def test_a_sphere_is_found_by_the_eye_on_its_side_and_dev_grows_with_its_azimuth():
    """Measured with this specification: area 0.036-0.039 in the seeing eye; cx 0.758 / 0.457 in the left eye at 30 / 70 degrees,
    0.242 / 0.543 in the right eye at -30 / -70 degrees, so dev = 0.242 at +-30 and 0.543 at +-70 degrees."""
    from flygym_amd.sensors import EYE_CAMERAS

    front = spec.front_edge(EYE_CAMERAS)
    dev = {}
    for az in AZIMUTHS:
        feat = _features(az)
        seeing, other = (0, 1) if az > 0 else (1, 0)
        print(f"azimuth {az:+.0f}: features (cy, cx, area) left {feat[0].tolist()} right {feat[1].tolist()}")
        assert feat[seeing, 2] > spec.DEFAULTS["area_threshold"] and feat[other, 2] == 0
        assert feat[other].tolist() == [0.5, 0.5, 0.0]
        dev[az] = 1.0 - feat[seeing, 1] if front[seeing] else feat[seeing, 1]
        assert 0.0 < dev[az] < 1.0
    assert dev[70.0] > dev[30.0] and dev[-70.0] > dev[-30.0]
    v = {az: spec.visual_speed(_features(az), front, **spec.DEFAULTS) for az in AZIMUTHS}
    for az in AZIMUTHS:                          # the side the sphere is on is slowed, the other is not: the fly turns towards it
        slow, fast = (0, 1) if az > 0 else (1, 0)
        assert v[az][slow] < 1.0 and v[az][fast] == 1.0
    # (with the default gain of 3 both azimuths already sit on v_min: 1 - 3 x 0.242 < 0.4; a gain of 1 tells them apart)
    assert v[70.0][0] <= v[30.0][0] == f32(0.4) and v[-70.0][1] <= v[-30.0][1] == f32(0.4)
    mild = {az: spec.visual_speed(_features(az), front, **{**spec.DEFAULTS, "visual_gain": 1.0}) for az in AZIMUTHS}
    assert mild[70.0][0] < mild[30.0][0] < 1 and mild[-70.0][1] < mild[-30.0][1] < 1


def test_what_the_eyes_do_not_see():
    behind = _features(150.0)
    assert (behind[:, 2] == 0).all()                                       # a sphere behind the fly: neither eye
    nothing = _readings(None)
    assert float((nothing[..., 0] + nothing[..., 1]).min()) > spec.DEFAULTS["obj_threshold"]
    assert _features(None).tolist() == [[0.5, 0.5, 0.0]] * 2               # no sphere: area exactly 0
    # a sphere of half the radius covers a quarter of the solid angle: 0.0097 of the eye, just below the default area_threshold —
    # the default tells a 2 mm sphere at 8 mm from a 1 mm one
    small = _features(30.0, radius=1.0)
    print(f"radius 1 mm at 8 mm: area {small[0, 2]:.4f}")
    assert 0.0 < small[0, 2] < spec.DEFAULTS["area_threshold"] and small[1, 2] == 0
    front = (1, 0)
    assert spec.visual_speed(small, front, **spec.DEFAULTS).tolist() == [1.0, 1.0]


def _rule_inputs(seed=5, n=400):
    rng = np.random.default_rng(seed)
    feat = np.empty((n, 2, 3), dtype=f32)
    feat[..., 0] = rng.random((n, 2))
    feat[..., 1] = rng.random((n, 2))
    feat[..., 2] = np.where(rng.random((n, 2)) < 0.6, rng.random((n, 2)) * 0.1, 0.0)
    odor = (rng.random((n, 3, 4)) * rng.choice([0.0, 1.0, 30.0], size=(n, 3, 1))).astype(f32)
    gains = np.array([1.5, -0.7, 0.25], dtype=f32)
    return feat, odor, gains


def _drive(feat, odor, gains, front=(1, 0), **over):
    p = {**spec.DEFAULTS, **over}
    v = spec.visual_speed(feat, front, **p)
    b = spec.odor_bias(odor, gains, **p) if odor is not None else np.zeros(feat.shape[0], dtype=f32)
    return spec.drive_from(v, b, **p), b


def test_the_mirror_scenario_swaps_the_two_drives_exactly():
    feat, odor, gains = _rule_inputs()
    # the mirrored fly: eyes swapped, each image flipped left-right (cx -> 1 - cx, which also swaps the frontal edges' roles),
    # odor sites swapped left <-> right.  cx is drawn on a grid of 2^-12 so that 1 - cx is exact.
    feat[..., 1] = np.round(feat[..., 1] * 4096) / 4096
    mirrored = feat[:, ::-1].copy()
    mirrored[..., 1] = f32(1) - mirrored[..., 1]
    d0, b0 = _drive(feat, odor, gains)
    d1, b1 = _drive(mirrored, odor[..., [1, 0, 3, 2]], gains)
    assert np.array_equal(b1, -b0) and np.array_equal(d1, d0[:, ::-1])
    assert (d0[:, 0] != d0[:, 1]).any()


def test_the_drive_is_monotone_in_dev_and_in_the_bias():
    dev = np.linspace(0, 1, 257).astype(f32)
    feat = np.tile(np.array([0.5, 0.5, 0.0], dtype=f32), (dev.size, 2, 1))
    feat[:, 0, 1], feat[:, 0, 2] = f32(1) - dev, 0.05                       # the left eye (frontal edge: last column) sees it
    left = spec.drive_from(spec.visual_speed(feat, (1, 0), **spec.DEFAULTS), np.zeros(dev.size, dtype=f32), **spec.DEFAULTS)
    assert (np.diff(left[:, 0]) <= 0).all() and left[0, 0] > left[-1, 0] and (left[:, 1] == 1).all()
    b = np.linspace(-6, 6, 1001).astype(f32)
    d = spec.drive_from(np.ones((b.size, 2), dtype=f32), b, **spec.DEFAULTS)
    assert (np.diff(d[:, 0]) <= 0).all() and (np.diff(d[:, 1]) >= 0).all()    # more odor on the left slows the left legs
    assert d[0, 0] == 1 and d[-1, 1] == 1 and d[-1, 0] < 0.25 and d[0, 1] < 0.25


def test_the_squash_is_odd_monotone_and_bounded():
    b = np.concatenate([np.linspace(0, 8, 4001), [1e3, 1e6, 3e18, 1e-20, 1e-30]]).astype(f32)
    q = spec.squash(b)
    assert np.array_equal(spec.squash(-b), -q)
    assert (np.abs(q) <= 1).all() and (np.abs(spec.squash(np.linspace(-50, 50, 2001).astype(f32))) < 1).all()
    assert (np.diff(q[:4001]) >= 0).all() and q[0] == 0
    assert np.isfinite(q[:-5]).all()


def test_absent_inputs_give_the_base_drive_and_the_clamps_hold():
    feat, odor, gains = _rule_inputs(n=16)
    table = np.zeros((7, 2), dtype=np.int16)
    f, b, d = spec.update(odor=odor * 0, gains=gains, base=0.9)
    assert (b == 0).all() and (d == f32(0.9)).all() and f.tolist() == [[[0.5, 0.5, 0.0]] * 2] * 16
    bright = np.full((16, 2, 7, 2), 0.5, dtype=f32)
    f, b, d = spec.update(omm=bright, table=table, height=9, width=9, base=0.9)
    assert (b == 0).all() and (d == f32(0.9)).all()
    # the ends: v clipped at v_min / v_max, the drive at drive_min / drive_max
    ends = np.tile(np.array([0.5, 0.5, 0.5], dtype=f32), (2, 2, 1))
    ends[0, 0, 1], ends[1, 0, 1] = 0.0, 1.0                                  # left eye: dev = 1 (far behind), dev = 0 (dead ahead)
    v = spec.visual_speed(ends, (1, 0), **{**spec.DEFAULTS, "v_max": 0.95})
    assert v[:, 0].tolist() == [f32(0.4), f32(0.95)]
    d = spec.drive_from(np.array([[0.4, 1.2]], dtype=f32), np.array([50.0], dtype=f32), **{**spec.DEFAULTS, "base": 1.1})
    assert d.tolist() == [[f32(0.2), f32(1.2)]]


def test_a_reading_exactly_at_the_threshold_is_not_dark():
    thr = f32(spec.DEFAULTS["obj_threshold"])
    omm = np.zeros((3, 5, 2), dtype=f32)
    omm[0, :, 0] = thr                                                       # at the threshold: not dark
    omm[1, :, 1] = np.nextafter(thr, f32(0))                                 # one ulp below, in the pale channel: dark
    omm[2, :, 0] = thr
    omm[2, 3, 0] = 0.0
    table = spec.centre_table(np.array([[1.5, 2.5], [3.5, 0.5], [6.0, 6.0], [7.25, 1.0], [0.5, 7.5]]))
    feat = spec.features(omm, table, 8, 8)
    assert feat[0].tolist() == [0.5, 0.5, 0.0]
    assert feat[1, 2] == 1.0 and feat[1, 1] == f32(np.mean([1.5, 3.5, 6.0, 7.25, 0.5]) / 8) and feat[1, 0] == f32(np.mean([2.5, 0.5, 6.0, 1.0, 7.5]) / 8)
    assert feat[2].tolist() == [f32(1.0 / 8), f32(7.25 / 8), f32(0.2)]
