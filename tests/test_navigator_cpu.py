"""The plume navigator's specification ``tests/navigator_spec.py`` against the properties its definition promises, the coverage its
input generator gives the GPU parity tests, and the ctypes mirror of ``nmf_navigator_params`` against the library (no GPU)."""
import ctypes
import dataclasses

import numpy as np
import pytest

import navigator_spec as spec
import plume_spec

from flygym_amd import _native
from flygym_amd.controllers import _NavigatorParams, navigator_constants

BASE = spec.Params(dt=0.05, threshold=0.1, decay_stop=0.75, decay_walk=0.5, decay_freq=0.875, inv_tau_freq=0.5, turn_ticks=3)
IDENTITY = np.array([[1.0, 0.0, 0.0, 0.0]], dtype=np.float32)


def _params(**over):
    return dataclasses.replace(BASE, **over)


def _odor(n, left=0.0, right=0.0):
    odor = np.zeros((n, 1, 4), dtype=np.float32)
    odor[:, 0, 2], odor[:, 0, 3] = left, right
    return odor


def _yaw(angle):
    return np.array([[np.cos(angle / 2), 0.0, 0.0, np.sin(angle / 2)]], dtype=np.float32)


def test_params_struct_matches_the_library():
    """The library loads without a GPU; the ctypes mirror has the layout it was compiled with."""
    _native.build()
    L = _native.lib()
    assert ctypes.sizeof(_NavigatorParams) == L.nmf_navigator_params_size() == 104
    for name in ("nmf_navigator_params_size", "nmf_navigator_create", "nmf_navigator_destroy", "nmf_navigator_reset",
                 "nmf_navigator_update", "nmf_navigator_field_ptr"):
        assert name in _native.exported_symbols() and hasattr(L, name)
    assert set(spec.Params.__dataclass_fields__) <= {name for name, _ in _NavigatorParams._fields_}


def test_constants_are_float32_roundings_of_float64_values():
    c = navigator_constants(**spec.PARITY_TIMES)
    assert c["turn_ticks"] == 3 and c["inv_tau_freq"] == np.float32(0.5)
    for name, tau in (("decay_stop", 0.2), ("decay_walk", 0.52), ("decay_freq", 2.0)):
        assert c[name].dtype == np.float32 and c[name] == np.float32(np.exp(-0.05 / tau)) == getattr(spec.PARITY, name)
    for bad in (dict(tick_s=0.0), dict(tau_walk=-1.0), dict(tau_freq=np.inf), dict(turn_duration=0.0), dict(turn_duration=1e4)):
        with pytest.raises(ValueError):
            navigator_constants(**{**spec.PARITY_TIMES, **bad})


def test_the_draws_are_the_plumes_hash_at_indices_8_to_10():
    seed, first = 0xDEADBEEF, 1000
    world, tick = np.arange(7), np.array([0, 1, 2, 3, 4, 5, 0xFFFFFFFF], dtype=np.uint32)
    u = spec.draws(seed, first + world, tick)
    assert u.dtype == np.float32 and u.shape == (3, 7)
    for m in range(3):
        ints = plume_spec.uniforms(seed, first + world, tick, 8 + m)
        assert np.array_equal(u[m], ints.astype(np.float64) * 2.0 ** -24)         # (24-bit integers: exact in float32)
        for plume_m in range(8):                                                   # (another stream than the wind noise's)
            assert not np.array_equal(ints, plume_spec.uniforms(seed, first + world, tick, plume_m))
    # the state machine consumes them: from WALK with p_stop = 1/2 and no turns, world w stops exactly when its u_0 < 1/2
    st = spec.State(64, _params(lambda_ws0=10.0, dlambda_ws=0.0, lambda_turn=0.0), seed=seed, first_world=first)
    st.update(_odor(64), np.zeros(2), np.repeat(IDENTITY, 64, axis=0))
    want = plume_spec.uniforms(seed, first + np.arange(64), 0, 8) < 2 ** 23
    assert np.array_equal(st.state == spec.STOP, want) and 10 < want.sum() < 54
    # and the second update draws at tick 1
    walking = st.state == spec.WALK
    st.update(_odor(64), np.zeros(2), np.repeat(IDENTITY, 64, axis=0))
    want = plume_spec.uniforms(seed, first + np.arange(64), 1, 8) < 2 ** 23
    assert np.array_equal((st.state == spec.STOP)[walking], want[walking])


def test_encounters_are_strict_upward_crossings():
    """Constant odor above the threshold is one encounter; a dip to the threshold itself and a rise is a second (s > threshold is
    strict); a NaN reading is never one."""
    thr = np.float32(0.1)
    st = spec.State(1, _params(threshold=thr))
    for _ in range(10):
        st.update(_odor(1, 0.2, 0.1), np.zeros(2), IDENTITY)
    assert st.encounters.tolist() == [1] and st.above.tolist() == [1]
    st.update(_odor(1, thr, 0.0), np.zeros(2), IDENTITY)                           # the sum equals the threshold: not above
    assert st.above.tolist() == [0] and st.encounters.tolist() == [1]
    st.update(_odor(1, 0.2, 0.1), np.zeros(2), IDENTITY)
    assert st.encounters.tolist() == [2] and st.above.tolist() == [1]
    # NaN in either antenna: no encounter, and not above
    st = spec.State(1, _params())
    for left, right in ((np.nan, 0.5), (0.5, np.nan), (np.inf, -np.inf), (np.nan, np.nan)):
        st.update(_odor(1, left, right), np.zeros(2), IDENTITY)
        assert st.encounters.tolist() == [0] and st.above.tolist() == [0] and not st.last["e"].any()
    assert st.k_stop.tolist() == [0.0] and st.freq.tolist() == [0.0]


def test_filters_decay_by_exactly_their_factor():
    p = _params()
    st = spec.State(1, p)
    st.update(_odor(1, 0.3, 0.3), np.zeros(2), IDENTITY)
    assert (st.k_stop[0], st.k_walk[0], st.freq[0]) == (1.0, 1.0, 0.5)
    for k in range(1, 12):                                                          # the odor stays: no further encounter
        before = st.snapshot()
        st.update(_odor(1, 0.3, 0.3), np.zeros(2), IDENTITY)
        assert st.k_stop[0] == before["k_stop"][0] * p.decay_stop == np.float32(0.75 ** k)
        assert st.k_walk[0] == before["k_walk"][0] * p.decay_walk == np.float32(0.5 ** k)
        assert st.freq[0] == before["freq"][0] * p.decay_freq
    assert st.encounters.tolist() == [1]


@pytest.mark.parametrize("turn_ticks", [1, 3, 7])
def test_a_turn_holds_its_drive_for_exactly_turn_ticks(turn_ticks):
    """p_turn = 1 and p_stop = 0: the first update starts a turn, the turn row stands for turn_ticks updates, then one update
    of the walk row, then the next turn."""
    p = _params(lambda_ws0=0.0, dlambda_ws=0.0, lambda_turn=1000.0, turn_ticks=turn_ticks, p_up_min=1.0, p_up_max=1.0,
                turn_drive=(0.25, 1.5))
    st = spec.State(1, p)
    rows = []
    for _ in range(2 * (turn_ticks + 1)):
        st.update(_odor(1), np.array([-1.0, 1.0]), IDENTITY)                       # upwind (1, -1) lies to the right of +x
        rows.append((int(st.state[0]), *st.drive[0].tolist()))
    turn, walk = (spec.TURN_RIGHT, 1.5, 0.25), (spec.WALK, 1.0, 1.0)
    assert rows == ([turn] * turn_ticks + [walk]) * 2
    assert st.ticks.tolist() == [2 * (turn_ticks + 1)]


def test_clamped_probabilities_alternate_walk_and_stop():
    p = _params(lambda_ws0=1e6, lambda_sw0=1e6, lambda_turn=0.0)
    st = spec.State(5, p, seed=3)
    seen = []
    for _ in range(8):
        st.update(_odor(5), np.zeros(2), np.repeat(IDENTITY, 5, axis=0))
        assert st.last["p_stop"].tolist() == [1.0] * 5 and st.last["p_walk"].tolist() == [1.0] * 5
        seen.append(st.state.tolist())
    assert seen == [[spec.STOP] * 5, [spec.WALK] * 5] * 4
    assert np.array_equal(st.drive, np.ones((5, 2), dtype=np.float32))
    # negative rates clamp to 0: nothing ever happens
    st = spec.State(5, _params(lambda_ws0=-5.0, lambda_turn=-1.0))
    for _ in range(20):
        st.update(_odor(5), np.zeros(2), np.repeat(IDENTITY, 5, axis=0))
    assert not st.state.any() and st.last["p_stop"].tolist() == [0.0] * 5


@pytest.mark.parametrize("p_up", [1.0, 0.0])
def test_turns_go_upwind_or_downwind_in_every_quadrant(p_up):
    """Winds from all four quadrants against headings in all four: with p_up = 1 the turn goes to the side the upwind direction
    (-wind) lies on, seen from the heading; with p_up = 0 to the other."""
    p = _params(lambda_ws0=0.0, dlambda_ws=0.0, lambda_turn=1000.0, p_up_min=p_up, p_up_max=p_up)
    for hq in range(4):
        yaw = 0.3 + hq * np.pi / 2
        for wq in range(4):
            wind_angle = 1.1 + wq * np.pi / 2
            wind = 25.0 * np.array([np.cos(wind_angle), np.sin(wind_angle)])
            st = spec.State(1, p, seed=hq * 4 + wq)
            st.update(_odor(1), wind, _yaw(yaw))
            upwind_left = np.sin(np.arctan2(-wind[1], -wind[0]) - yaw) > 0
            assert st.state[0] == (spec.TURN_LEFT if upwind_left == (p_up == 1.0) else spec.TURN_RIGHT), (hq, wq)
            assert st.remaining[0] == p.turn_ticks and bool(st.last["upwind"][0]) == (p_up == 1.0)
    # a NaN in the wind: cross > 0 is false, as if upwind lay to the right
    for wind in ((np.nan, 1.0), (1.0, np.nan), (np.inf, np.inf), (np.nan, np.nan)):
        st = spec.State(1, p)
        st.update(_odor(1, np.nan, np.inf), np.array(wind), _yaw(0.3))
        assert st.state[0] == (spec.TURN_RIGHT if p_up == 1.0 else spec.TURN_LEFT)
        assert all(np.isfinite(getattr(st, name)).all() for name in spec.FIELDS)
    st = spec.State(1, p)
    st.update(_odor(1), np.array([-1.0, 0.5]), np.full((1, 4), np.nan, dtype=np.float32))   # an attitude that is not a number likewise
    assert st.state[0] == (spec.TURN_RIGHT if p_up == 1.0 else spec.TURN_LEFT)


def test_stationary_occupancy_of_the_two_state_chain():
    """No turns and no odor: WALK and STOP form a two-state Markov chain with p_stop = 0.2 and p_walk = 0.3 per update, whose
    stationary share of STOP is p_stop / (p_stop + p_walk) = 0.4 and whose lag-1 autocorrelation is rho = 1 - p_stop - p_walk.  The
    mean of n T correlated samples has the variance pi (1 - pi) / (n T) x (1 + rho) / (1 - rho); 256 worlds x 400 updates after
    50 updates of burn-in (rho^50 = 1e-15) put five standard errors at 0.013."""
    n, T, burn = 256, 400, 50
    st = spec.State(n, _params(lambda_ws0=4.0, dlambda_ws=0.0, lambda_sw0=6.0, dlambda_sw=0.0, lambda_turn=0.0), seed=11)
    quat = np.repeat(IDENTITY, n, axis=0)
    stopped = 0
    for k in range(burn + T):
        st.update(_odor(n), np.zeros(2), quat)
        if k >= burn:
            stopped += int((st.state == spec.STOP).sum())
    p_stop, p_walk = float(st.last["p_stop"][0]), float(st.last["p_walk"][0])
    assert abs(p_stop - 0.2) < 1e-7 and abs(p_walk - 0.3) < 1e-7
    pi, rho = p_stop / (p_stop + p_walk), 1.0 - p_stop - p_walk
    bar = 5.0 * np.sqrt(pi * (1 - pi) / (n * T) * (1 + rho) / (1 - rho))
    share = stopped / (n * T)
    print(f"share of STOP {share:.4f}, stationary {pi:.4f}, five standard errors {bar:.4f}")
    assert bar < 0.02
    assert abs(share - pi) <= bar
    assert set(np.unique(st.state)) == {spec.WALK, spec.STOP}


@pytest.mark.parametrize("shared_wind", [False, True])
@pytest.mark.parametrize("n,T", spec.CASES)
def test_the_parity_inputs_cover_every_transition(n, T, shared_wind):
    """What ``tests/test_navigator_gpu.py`` relies on, asserted on the specification alone: in each of its runs every one of the
    six transitions occurs at least 3 times, upwind and downwind choices at least 3 times each, at least 3 turn decisions are
    taken at a p_up strictly between its bounds, and the inputs hold values that are not finite."""
    snaps, cover = spec.reference_run(n, T, shared_wind)
    print(n, T, shared_wind, cover)
    assert len(snaps) == T
    for name in ("walk_stop", "stop_walk", "walk_left", "walk_right", "left_walk", "right_walk", "upwind", "downwind", "p_up_inside"):
        assert cover[name] >= 3, (name, cover)
    assert cover["encounters"] >= 3 and (snaps[-1]["ticks"] == T).all()
    assert all(np.isfinite(snaps[-1][name]).all() for name in spec.FIELDS)
    odor, wind, _ = spec.input_run(n, T)
    assert not np.isfinite(odor[:, :, 1, 2:]).all() and not np.isfinite(wind).all()
    assert np.isnan(odor).any() and np.isposinf(odor).any() and np.isneginf(odor).any()
    # world n - 1 is the same world in every batch size
    last = spec.input_run(1, T)
    for a, b in zip(spec.input_run(n, T), last):
        assert np.array_equal(a[:, -1], b[:, 0], equal_nan=True)
