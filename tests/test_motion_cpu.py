"""The motion-vision specification (``tests/motion_spec.py``) against what it promises, and ``Retina.motion_pairs`` — no GPU.

Drifting sine gratings on the default retina: wavelength six lattice pitches, contrast 0.4 about 0.5, ``dt`` = 2 ms, 1500 ticks, the
flow averaged over the second half.  Run once for all directions and temporal frequencies (one world each), shared and read-only."""
import ctypes
import functools

import numpy as np
import pytest

import motion_spec as spec

f32 = np.float32
DT, TICKS = 0.002, 1500
DIRECTIONS = {"+x": (1.0, 0.0), "-x": (-1.0, 0.0), "+y": (0.0, 1.0), "-y": (0.0, -1.0)}
FREQUENCIES = (0.25, 2.0, 64.0)


@functools.lru_cache(maxsize=None)
def _retina():
    from flygym_amd.sensors import Retina

    return Retina()


@functools.lru_cache(maxsize=None)
def _pairs():
    pairs, weights = _retina().motion_pairs()
    pairs.setflags(write=False); weights.setflags(write=False)
    return pairs, weights


def _pitch(centres):
    d = np.hypot(*(centres[None] - centres[:, None]).transpose(2, 0, 1))
    np.fill_diagonal(d, np.inf)
    return float(np.median(d.min(axis=1)))


@functools.lru_cache(maxsize=None)
def _gratings():
    """Worlds: every direction at every frequency (direction-major), then a static grating.  Returns ``dict(flow32, flow64
    (worlds, 2, 2): means over the second half; static: every output of every tick of the static world; worlds)``."""
    r = _retina()
    c = r.ommatidia_centres()
    pairs, weights = _pairs()
    lam = 6.0 * _pitch(c)
    worlds = [(d, f) for d in DIRECTIONS for f in FREQUENCIES] + [("+x", 0.0)]
    along = np.array([c @ np.array(DIRECTIONS[d]) for d, _ in worlds])                    # (worlds, n_omm)
    freq = np.array([f for _, f in worlds])[:, None]
    pale = r.pale_mask != 0
    n = len(worlds)
    s32, s64 = spec.new_state(n, r.num_ommatidia), spec.new_state(n, r.num_ommatidia, np.float64)
    acc32, acc64, static = np.zeros((n, 2, 2)), np.zeros((n, 2, 2)), []
    for k in range(TICKS):
        x = (0.5 + 0.4 * np.sin(2.0 * np.pi * (along / lam - freq * (k * DT)))).astype(f32)      # drifts along its direction
        x = np.stack([x, x], axis=1)                                                      # both eyes see the same image
        omm = np.stack([np.where(pale, 0, x), np.where(pale, x, 0)], axis=-1).astype(f32)
        out = spec.update(s32, omm, pairs, weights, dt=DT, base=np.full((n, 2), 0.9, dtype=f32))
        flow64 = spec.update64(s64, omm, pairs, weights, dt=DT)
        static.append({name: v[-1].copy() for name, v in out.items()})
        if k >= TICKS // 2:
            acc32 += out["flow"]
            acc64 += flow64
    half = TICKS - TICKS // 2
    return dict(flow32=acc32 / half, flow64=acc64 / half, static=static, worlds=worlds)


def _mean_flow(direction, frequency):
    g = _gratings()
    return g["flow32"][g["worlds"].index((direction, frequency))]


def test_the_default_retinas_pair_list():
    r = _retina()
    pairs, weights = r.motion_pairs()
    assert pairs.dtype == np.int32 and weights.dtype == f32 and pairs.shape == weights.shape == (2070, 2)
    assert (pairs[:, 0] < pairs[:, 1]).all() and pairs.min() == 0 and pairs.max() == 720
    order = np.lexsort((pairs[:, 1], pairs[:, 0]))
    assert np.array_equal(order, np.arange(2070))                                         # ascending (a, b), no pair twice
    assert len({tuple(p) for p in pairs.tolist()}) == 2070
    partners = np.bincount(pairs.ravel(), minlength=721)
    assert partners.min() == 3 and partners.max() == 6
    assert np.abs(np.hypot(weights[:, 0], weights[:, 1]) - 1).max() < 2e-7
    # three axes: the angles of the unit vectors, modulo 180 degrees, cluster around 30, 90 and 150 degrees (a flat-top lattice)
    angle = np.degrees(np.arctan2(weights[:, 1].astype(np.float64), weights[:, 0].astype(np.float64))) % 180.0
    assert np.abs(angle % 60.0 - 30.0).max() < 2.0 and np.bincount((angle // 60.0).astype(int)).tolist() == [690, 690, 690]
    again = r.motion_pairs()
    assert np.array_equal(again[0], pairs) and np.array_equal(again[1].view(np.int32), weights.view(np.int32))       # deterministic
    want = spec.motion_pairs(r.ommatidia_centres())
    assert np.array_equal(want[0], pairs) and np.array_equal(want[1].view(np.int32), weights.view(np.int32))


def test_pair_lists_the_kernel_cannot_hold_are_refused():
    from flygym_amd.sensors import Retina

    assert Retina(id_map=np.ones((3, 3), dtype=np.int16)).motion_pairs()[0].shape == (0, 2)           # one ommatidium: no pair
    square = Retina(id_map=np.arange(1, 1025, dtype=np.int16).reshape(32, 32))
    assert square.motion_pairs(reach=1.25)[0].shape == (2 * 32 * 31, 2)                             # the four-neighbour lattice
    with pytest.raises(ValueError, match="3072"):
        square.motion_pairs(reach=1.5)                                                                 # with the diagonals: 3906
    with pytest.raises(ValueError, match="1024"):
        Retina(id_map=np.arange(1, 1026, dtype=np.int16).reshape(25, 41)).motion_pairs()


def test_the_sign_of_the_flow_follows_the_drift():
    """Measured with this specification (H along +x, mean of the second half): 0.25 Hz 1.55e-2 (-x: -1.72e-2: the half holds
    three eighths of a period), 2 Hz 4.56e-2, 64 Hz 4.75e-3; exactly 0 across the drift."""
    for f in FREQUENCIES:
        px, mx, py, my = (_mean_flow(d, f) for d in ("+x", "-x", "+y", "-y"))
        print(f"{f} Hz: +x {px[0].tolist()} -x {mx[0].tolist()} +y {py[0].tolist()} -y {my[0].tolist()}")
        assert (px[:, 0] > 0).all() and (mx[:, 0] < 0).all() and (py[:, 1] > 0).all() and (my[:, 1] < 0).all()
        if f >= 2.0:                 # (the averaged half holds whole periods: the two directions mirror each other)
            assert np.allclose(mx[:, 0], -px[:, 0], rtol=0.02) and np.allclose(my[:, 1], -py[:, 1], rtol=0.02)
        assert (np.abs(px[:, 1]) < 0.02 * px[:, 0]).all() and (np.abs(py[:, 0]) < 0.02 * py[:, 1]).all()       # nothing across the drift
        assert np.array_equal(px[0], px[1])                                                # (the eyes saw the same image)


def test_the_response_peaks_between_the_slow_and_the_fast_grating():
    for d, c in (("+x", 0), ("+y", 1)):
        low, mid, high = (_mean_flow(d, f)[0, c] for f in FREQUENCIES)
        assert mid > low > 0 and mid > high > 0, (d, low, mid, high)


def test_a_static_grating_gives_exactly_nothing():
    for k, out in enumerate(_gratings()["static"]):
        assert not out["sums"].any() and not out["flow"].any() and out["rotation"] == 0 and out["translation"] == 0, k
        assert out["drive"].tolist() == [f32(0.9)] * 2, k
        assert not np.signbit(out["rotation"]) and not np.signbit(out["translation"])


def test_the_specification_stays_close_to_its_float64_restatement():
    """The largest deviation of the mean H and V over all gratings, measured: 1.25e-7 (the responses are 5e-3 to 5e-2).  The bar is
    four times that: the fixed-point resolution (2^-16 a term, 2^-17 rounding error at most, averaged over 2070 pairs and 750
    ticks) and the float32 filter rounding vary with the phase of the grating."""
    g = _gratings()
    worst = float(np.abs(g["flow32"] - g["flow64"]).max())
    print(f"float32 fixed-point specification against float64: max |difference| of the mean flow {worst:.3e}")
    assert worst < 4 * 1.25e-7


def _flows(h_left, h_right):
    flow = np.zeros((len(h_left), 2, 2), dtype=f32)
    flow[:, 0, 0], flow[:, 1, 0] = h_left, h_right
    flow[..., 1] = 0.37                                                                    # (V takes no part)
    return flow


def test_rotation_and_drive_on_hand_made_flows():
    p = {**spec.DEFAULTS, "gain": 10.0}
    h = np.array([0.0, 0.01, -0.01, 0.05, 1e3], dtype=f32)
    # front_edge (1, 0): the left image's last column faces forward, so front-to-back is -H there and +H in the right eye
    rot, tra, d = spec.optomotor(_flows(-h, -h), (1, 0), **p)                        # left eye sees ftb h, right eye -h
    assert np.array_equal(rot, (h + h).astype(f32)) and (tra == 0).all()
    q = np.array([float(f32(10.0) * r) / float(f32(1) + abs(f32(10.0) * r)) for r in rot], dtype=f32)
    assert np.array_equal(d[:, 1], np.where(q >= 0, f32(1), d[:, 1])) and d[0].tolist() == [1.0, 1.0]
    assert np.array_equal(d[:, 0], np.fmax((f32(1) - f32(0.8) * np.fmax(q, f32(0))).astype(f32), f32(0.2)))
    assert d[1, 0] < 1 and d[1, 1] == 1 and d[2, 1] < 1 and d[2, 0] == 1                   # counter-clockwise slows the left side
    assert d[2].tolist() == d[1, ::-1].tolist()
    assert 0.9999 < q[4] < 1 and f32(0.2) < d[4, 0] < 0.2001                             # q saturates below 1: 1 - delta is never reached
    _, _, low = spec.optomotor(_flows(-h, -h), (1, 0), **{**p, "drive_min": 0.5})
    assert low[4].tolist() == [0.5, 1.0] and low[1, 0] == d[1, 0] > 0.5                   # the lower clamp
    rot2, tra2, d2 = spec.optomotor(_flows(h, h), (0, 1), **p)                       # the other orientation of both cameras
    assert np.array_equal(rot2, rot) and np.array_equal(d2, d)
    rot3, tra3, _ = spec.optomotor(_flows(-h, h), (1, 0), **p)                       # both eyes front to back: translation
    assert (rot3 == 0).all() and np.array_equal(tra3, (h + h).astype(f32)) and not np.signbit(rot3).any()
    # base as a tensor, and the upper clamp
    base = np.array([[1.5, 0.5]] * 5, dtype=f32)
    _, _, d4 = spec.optomotor(_flows(-h, -h), (1, 0), **{**p, "base": base})
    assert d4[0].tolist() == [f32(1.2), f32(0.5)] and d4[4].tolist() == [f32(1.5 * (1 - 0.8 * q[4])), f32(0.5)]
    _, _, d5 = spec.optomotor(_flows(-h, -h), (1, 0), **{**p, "delta": 0.0})
    assert (d5 == 1).all()


def test_a_reset_world_starts_again_and_the_others_are_untouched():
    rng = np.random.default_rng(3)
    n, n_omm = 5, 40
    pairs = np.stack([np.arange(n_omm - 1), np.arange(1, n_omm)], axis=-1).astype(np.int32)
    weights = np.tile(np.array([[1.0, 0.0]], dtype=f32), (n_omm - 1, 1))
    frames = rng.random((4, n, 2, n_omm, 2)).astype(f32)
    frames[..., 1] = 0
    a, b = spec.new_state(n, n_omm), spec.new_state(n, n_omm)
    for k in range(3):
        spec.update(a, frames[k], pairs, weights, dt=DT)
        spec.update(b, frames[k], pairs, weights, dt=DT)
    assert not a["fresh"].any()
    mask = np.array([0, 1, 0, 0, 1], dtype=np.uint8)
    spec.reset(a, mask)
    assert a["fresh"].tolist() == [False, True, False, False, True] and np.array_equal(a["fast"], b["fast"])
    out_a = spec.update(a, frames[3], pairs, weights, dt=DT)
    out_b = spec.update(b, frames[3], pairs, weights, dt=DT)
    first = spec.update(spec.new_state(n, n_omm), frames[3], pairs, weights, dt=DT)
    kept, again = mask == 0, mask != 0
    for name in out_a:
        assert np.array_equal(out_a[name][kept], out_b[name][kept]) and np.array_equal(out_a[name][again], first[name][again]), name
    assert not first["flow"].any()                                  # (a first update has hp = 0: no flow yet)
    assert out_b["flow"][kept].any() and not np.array_equal(a["fast"][again], b["fast"][again])
    assert np.array_equal(a["fast"][kept], b["fast"][kept]) and np.array_equal(a["slow"][kept], b["slow"][kept])


def test_the_coefficients_are_rounded_once():
    assert spec.coefficient(0.002, 0.035) == f32(1.0 - np.exp(-0.002 / 0.035)) and 0.0555 < spec.coefficient(0.002, 0.035) < 0.0556
    assert 0.0132 < spec.coefficient(0.002, 0.15) < 0.0133


def test_the_params_mirror_has_the_librarys_size():
    from flygym_amd import _native
    from flygym_amd._handle import check_params
    from flygym_amd.sensors import _MotionParams

    assert ctypes.sizeof(_MotionParams) == 36
    check_params(_MotionParams, "nmf_motion_params_size", "sensors.py")
    assert _native.lib().nmf_motion_params_size() == 36
