"""The path integrator's specification ``tests/odometry_spec.py`` against the properties its definition promises,
``PathIntegrator.calibrate`` against planted coefficients, and the ctypes mirror of ``nmf_odometry_params`` against the library
(no GPU)."""
import ctypes

import numpy as np
import pytest

import odometry_spec as spec

from flygym_amd import _native
from flygym_amd.sensors import PathIntegrator, _OdometryParams

NSEG, ROOT, TIPS = 8, 0, np.arange(1, 7)


def _poses(root_pos, yaw, tips_world):
    """Batch arrays of one world: the root at ``root_pos`` yawed by ``yaw``, the six tips at ``tips_world`` (6, 3)."""
    xpos = np.zeros((1, NSEG, 3), dtype=np.float32)
    xquat = np.zeros((1, NSEG, 4), dtype=np.float32)
    xquat[..., 0] = 1
    xpos[0, ROOT] = root_pos
    xpos[0, TIPS] = tips_world
    xquat[0, ROOT] = [np.cos(yaw / 2), 0, 0, np.sin(yaw / 2)]
    return xpos.reshape(1, -1), xquat.reshape(1, -1)


def _sensors(on, force=(0.0, 0.0, 1.0)):
    sd = np.zeros((1, 6, 16), dtype=np.float32)
    sd[0, :, 0] = np.asarray(on, dtype=np.float32)
    sd[0, :, 1:4] = force
    return sd.reshape(1, 96)


def test_params_struct_matches_the_library():
    """The library loads without a GPU; the ctypes mirror has the layout it was compiled with."""
    _native.build()
    L = _native.lib()
    assert ctypes.sizeof(_OdometryParams) == L.nmf_odometry_params_size() == 56
    for name in ("nmf_odometry_params_size", "nmf_odometry_create", "nmf_odometry_destroy", "nmf_odometry_reset", "nmf_odometry_update",
                 "nmf_odometry_field_ptr"):
        assert name in _native.exported_symbols() and hasattr(L, name)


def test_straight_walk_closed_form():
    """Six legs always in contact, their tips fixed in the world while the body translates at v dt = 0.04 per update along its own x
    axis at heading theta0; disp_coef = 1/6 each.  After K = 400 updates with a window of W = 5 the estimate has moved
    (K - W) v dt along (cos theta0, sin theta0).  The only rounding of any size is that of the float32 body-frame coordinate — two
    differences, three products and two sums of values up to the largest |tip - root| component, then the difference of two
    samples — so the bar is K x 4 ulp32 of that component (1.5e-3 here)."""
    K, W, step, theta0 = 400, 5, 0.04, 0.75                                    # (0.75 is a float32: the heading is exact)
    rng = np.random.default_rng(1)
    tips = np.concatenate([rng.uniform(-1.5, 1.5, (6, 2)), np.zeros((6, 1))], axis=1)
    coef = np.zeros(14)
    coef[6:12] = 1.0 / 6.0
    st = spec.State(1, W, coefficients=coef)
    st.reset(pose=np.array([[0.0, 0.0, theta0]]))
    direction = np.array([np.cos(theta0), np.sin(theta0)])
    reach = 0.0
    for k in range(K):
        root = np.array([*(k * step * direction), 1.0])
        reach = max(reach, float(np.abs(tips - root).max()))
        st.update(*_poses(root, theta0, tips), _sensors(np.ones(6)), ROOT, TIPS)
    bar = K * 4 * float(np.spacing(np.float32(reach)))
    length = (K - W) * step
    err_length = abs(float(st.moved[0]) - length)
    err_pos = float(np.abs(st.position[0] - length * direction).max())
    print(f"straight walk: length error {err_length:.3e}, position error {err_pos:.3e}, bar {bar:.3e}")
    assert reach > 8.0                                                          # (the body walks well away from the tips)
    assert err_length <= bar and err_pos <= bar
    assert st.heading[0] == theta0 and st.count[0] == K
    np.testing.assert_allclose(st.home[0], [-length, 0.0], atol=bar)            # the origin lies straight behind


def test_swing_and_touchdown_add_nothing():
    """One world whose legs all slide back 0.5 per update.  A leg adds a stride only while it is on the ground in this update and
    the previous one: not in the priming update, not during swing, and not in the update after touchdown."""
    on = [1, 1, 1, 0, 0, 1, 1, 1]                                              # swing in updates 3 and 4, touchdown in 5
    want = [0.0, 0.5, 1.0, 1.0, 1.0, 1.0, 1.5, 2.0]
    st = spec.State(1, 3)
    for k, (c, total) in enumerate(zip(on, want)):
        st.update_from(np.full((1, 6), 10.0 - 0.5 * k, dtype=np.float32), np.full((1, 6), bool(c)))
        assert np.array_equal(st.total[0], np.full(6, total)), k
        assert st.count[0] == k + 1
    # the window strides: the total now minus the total three updates ago
    assert np.array_equal(st.win[0], np.full(6, 2.0 - 1.0))
    # found > 0 with a force under a non-zero threshold is no contact; thr == 0 takes every found > 0
    sd = _sensors(np.ones(6), force=(0.3, 0.0, 0.4))                            # |F| = 0.5
    assert spec.contacts(sd, [0, 0.4, 0.6, 0, 0.4, 0.6]).tolist() == [[True, True, False, True, True, False]]
    assert not spec.contacts(_sensors(np.zeros(6)), np.zeros(6)).any()


@pytest.mark.parametrize("window", [1, 3, 8])
def test_the_estimate_starts_at_exactly_count_equal_window(window):
    """With disp_bias = window the displacement increment of a valid update is 1: the position stands still through the updates
    with count < window and moves by one from the update with count == window on."""
    coef = np.zeros(14)
    coef[13] = float(window)
    st = spec.State(2, window, coefficients=coef)
    for k in range(2 * window + 3):
        assert st.count.tolist() == [k, k]
        st.update_from(np.zeros((2, 6), dtype=np.float32), np.ones((2, 6), dtype=bool))
        assert st.position[:, 0].tolist() == [max(0, k + 1 - window)] * 2, k
        assert st.moved.tolist() == [max(0, k + 1 - window)] * 2
    # a masked reset starts the count, and so the wait, again for that world alone
    st.reset(mask=[True, False], pose=np.array([[5.0, 0.0, 0.0], [9.0, 9.0, 9.0]]))
    for k in range(window + 1):
        st.update_from(np.zeros((2, 6), dtype=np.float32), np.ones((2, 6), dtype=bool))
    assert st.position[:, 0].tolist() == [6.0, 2 * window + 3 - window + window + 1]


def test_heading_stays_wrapped_across_pi():
    for rate in (0.7, -0.7):
        coef = np.zeros(14)
        coef[12] = rate
        st = spec.State(1, 1, coefficients=coef)
        seen, crossings, angle = [], 0, 0.0
        for k in range(60):
            before = float(st.heading[0])
            st.update_from(np.zeros((1, 6), dtype=np.float32), np.ones((1, 6), dtype=bool))
            now = float(st.heading[0])
            if k >= 1:
                angle += rate
            assert -np.pi <= now <= np.pi
            assert abs(np.angle(np.exp(1j * (now - angle)))) < 1e-12          # the same direction as the unwrapped sum
            crossings += int(abs(now - before) > np.pi)
            seen.append(now)
        assert crossings >= 5 and min(seen) < -np.pi + 0.7 and max(seen) > np.pi - 0.7
    assert spec.wrap(np.array([np.pi, -np.pi, 3 * np.pi + 0.25, 0.0])).tolist() == pytest.approx([np.pi, -np.pi, -np.pi + 0.25, 0.0], abs=1e-15)


def test_calibrate_recovers_planted_coefficients():
    """Traces built from planted coefficients: the heading and the position of tick k are those of tick k - window plus the model's
    prediction, so the least-squares problem has an exact solution, found to 1e-9 relative.  The headings are stored wrapped."""
    rng = np.random.default_rng(4)
    T, n, W = 90, 5, 7
    win = rng.uniform(0.2, 2.0, (T, n, 6))
    a, hb = np.array([0.31, -0.12, 0.07]), 0.02
    b, db = np.array([0.45, 0.21, 0.33]), -0.05
    dh = (win[..., :3] - win[..., 3:]) @ a + hb
    dd = (win[..., :3] + win[..., 3:]) @ b + db
    assert np.abs(dh).max() < np.pi and dd.min() > 0
    pose = np.zeros((T, n, 3))
    pose[:W] = rng.uniform(-1, 1, (W, n, 3))
    along = rng.uniform(-np.pi, np.pi, (T, n))
    for k in range(W, T):
        pose[k, :, 2] = pose[k - W, :, 2] + dh[k]
        pose[k, :, :2] = pose[k - W, :, :2] + dd[k][:, None] * np.stack([np.cos(along[k]), np.sin(along[k])], axis=1)
    pose[..., 2] = np.angle(np.exp(1j * pose[..., 2]))
    coef, r2_h, r2_d = PathIntegrator.calibrate(win, pose, W)
    want = np.concatenate([a, -a, b, b, [hb, db]])
    assert coef.shape == (14,) and coef.dtype == np.float64
    np.testing.assert_allclose(coef, want, rtol=1e-9, atol=0)
    assert r2_h > 1 - 1e-12 and r2_d > 1 - 1e-12
    # the device's rule with these coefficients reproduces the targets: (bias + sum coef win) / window per update
    st = spec.State(1, W, coefficients=coef)
    assert np.isclose((st.coef[12] + st.coef[:6] @ win[20, 0]), dh[20, 0], rtol=1e-9)
    with pytest.raises(ValueError):
        PathIntegrator.calibrate(win[:W], pose[:W], W)
    with pytest.raises(ValueError):
        PathIntegrator.calibrate(win, pose[:, :, :2], W)
