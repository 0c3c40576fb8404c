"""The rule-based controller's host half and its specification ``tests/rules_spec.py`` (no GPU): the rule matrices, the swing runs,
the properties the model promises, the coverage the drive schedule gives the GPU parity tests, and the ctypes mirror of
``nmf_rules_params`` against the library.  The kernel is tested against the specification in ``tests/test_rules_gpu.py``."""
import ctypes

import numpy as np
import pytest

import plume_spec
import rules_spec as spec

from flygym_amd import _native
from flygym_amd.anatomy import LEGS
from flygym_amd.controllers import RULE_NAMES, RULE_WEIGHTS, _RulesParams, default_rules_graph, rule_matrices, swing_runs

# rule 1: anterior -> posterior neighbour; rule 2: posterior -> anterior neighbour and both ways across each pair; rule 3: anterior ->
# posterior neighbour and both ways across each pair
EDGES = {
    "rule1": [("lf", "lm"), ("lm", "lh"), ("rf", "rm"), ("rm", "rh")],
    "rule2_ipsi": [("lm", "lf"), ("lh", "lm"), ("rm", "rf"), ("rh", "rm")],
    "rule2_contra": [("lf", "rf"), ("rf", "lf"), ("lm", "rm"), ("rm", "lm"), ("lh", "rh"), ("rh", "lh")],
    "rule3_ipsi": [("lf", "lm"), ("lm", "lh"), ("rf", "rm"), ("rm", "rh")],
    "rule3_contra": [("lf", "rf"), ("rf", "lf"), ("lm", "rm"), ("rm", "lm"), ("lh", "rh"), ("rh", "lh")],
}
WEIGHTS = {"rule1": -10.0, "rule2_ipsi": 2.5, "rule2_contra": 1.0, "rule3_ipsi": 3.0, "rule3_contra": 2.0}


def _by_hand(edges, weights):
    out = np.zeros((3, 6, 6), dtype=np.float32)
    for name, pairs in edges.items():
        for src, tgt in pairs:
            out[int(name[4]) - 1, LEGS.index(src), LEGS.index(tgt)] += np.float32(weights[name])
    return out


def test_rule_matrices():
    assert tuple(LEGS) == ("lf", "lm", "lh", "rf", "rm", "rh") and RULE_WEIGHTS == WEIGHTS and tuple(EDGES) == RULE_NAMES
    W = rule_matrices()
    assert W.dtype == np.float32 and W.shape == (3, 6, 6)
    assert np.array_equal(W, _by_hand(EDGES, WEIGHTS))
    assert {k: sorted(v) for k, v in default_rules_graph().items()} == {k: sorted(v) for k, v in EDGES.items()}
    assert [int((W[r] != 0).sum()) for r in range(3)] == [4, 10, 10]
    assert W[0, LEGS.index("lf"), LEGS.index("lm")] == -10 and W[0, LEGS.index("lm"), LEGS.index("lf")] == 0     # [source][target]
    assert not np.diagonal(W, axis1=1, axis2=2).any()
    # an overridden weight, an overridden edge list
    assert np.array_equal(rule_matrices(weights={"rule2_contra": 0.25}), _by_hand(EDGES, {**WEIGHTS, "rule2_contra": 0.25}))
    only = {**EDGES, "rule3_contra": [("rf", "lf")]}
    assert np.array_equal(rule_matrices(rules_graph={"rule3_contra": [("rf", "lf")]}), _by_hand(only, WEIGHTS))
    assert not rule_matrices(rules_graph={name: [] for name in RULE_NAMES}).any()
    for bad in (dict(weights={"rule4": 1.0}), dict(rules_graph={"rule2": []}), dict(weights={"rule1": float("nan")}),
                dict(rules_graph={"rule1": [("lf", "xx")]}), dict(rules_graph={"rule1": [("lf",)]})):
        with pytest.raises(ValueError):
            rule_matrices(**bad)


def _stance(n_bins, swing_bins):
    """A stance table whose leg l swings in the bins ``swing_bins[l]``."""
    stance = np.ones((n_bins, 6), dtype=bool)
    for leg, bins in enumerate(swing_bins):
        stance[list(bins), leg] = False
    return stance


def test_swing_runs():
    start, length = swing_runs(_stance(10, [(2, 3, 4), (8, 9, 0, 1), (1, 2, 5, 6), (0,), (9,), (0, 1, 4, 5, 6, 8, 9)]))
    assert start.dtype == np.int32 and length.dtype == np.int32
    # a plain run; a run that wraps the end of the table; two runs of equal length: the lower start; single bins at either end;
    # of runs 8 9 0 1 (wrapping) and 4 5 6 the longer
    assert start.tolist() == [2, 8, 1, 0, 9, 8] and length.tolist() == [3, 4, 2, 1, 1, 4]
    # equal lengths where one run wraps: the one that STARTS at the lower bin is the one inside the table
    start, length = swing_runs(_stance(8, [(7, 0), (7, 0), (7, 0), (7, 0), (7, 0), (7, 0, 3, 4)]))
    assert start.tolist() == [7, 7, 7, 7, 7, 3] and length.tolist() == [2] * 6
    with pytest.raises(ValueError, match="swing in every bin"):
        swing_runs(_stance(6, [range(6), (1,), (1,), (1,), (1,), (1,)]))
    with pytest.raises(ValueError, match="stance in every bin"):
        swing_runs(_stance(6, [(1,), (1,), (), (1,), (1,), (1,)]))
    with pytest.raises(ValueError):
        swing_runs(np.ones((6, 5), dtype=bool))


def test_params_struct_matches_the_library():
    """The library loads without a GPU; the ctypes mirror has the layout it was compiled with."""
    from flygym_amd.controllers import RuleBasedController, TripodCPG, __all__ as exported

    _native.build()
    L = _native.lib()
    assert ctypes.sizeof(_RulesParams) == L.nmf_rules_params_size() == 44
    for name in ("nmf_rules_params_size", "nmf_rules_create", "nmf_rules_destroy", "nmf_rules_reset", "nmf_rules_field_ptr",
                 "nmf_rules_advance"):
        assert name in _native.exported_symbols() and hasattr(L, name)
    assert {"RuleBasedController", "rule_matrices", "swing_runs"} <= set(exported) and issubclass(RuleBasedController, TripodCPG)
    # refusals that need no device
    assert L.nmf_rules_advance(None, 1, None, 1, None) != 0 and b"null controller" in L.nmf_last_error()
    assert L.nmf_rules_reset(None, None, None) != 0 and b"null controller" in L.nmf_last_error()
    assert not L.nmf_rules_create(None, None, None, None, None, None, None) and b"null batch" in L.nmf_last_error()
    assert not L.nmf_rules_field_ptr(None, 0, None)
    L.nmf_rules_destroy(None)


def test_the_draw_is_the_plumes_hash_at_an_index_of_its_own():
    seed, first = 0xDEADBEEF, 1000
    world, tick = first + np.arange(7), np.array([0, 1, 2, 3, 4, 5, 0xFFFFFFFF], dtype=np.uint32)
    u = spec.draw(seed, world, tick)
    assert u.dtype == np.uint64 and (u < 2 ** 32).all() and len(set(u.tolist())) == 7
    assert np.array_equal(u >> np.uint64(8), plume_spec.uniforms(seed, world, tick, spec.DRAW))
    assert spec.DRAW == 11                                   # the wind noise draws at 0..7, the navigator at 8..10
    # the pick is uniform over the eligible legs: 4096 worlds at tick 0, six eligible legs each
    picks = (spec.draw(3, np.arange(4096), 0) * np.uint64(6)) >> np.uint64(32)
    counts = np.bincount(picks.astype(np.int64), minlength=6)
    assert counts.sum() == 4096 and counts.min() > 4096 / 6 - 5 * np.sqrt(4096 * 5 / 36)      # five standard deviations


def _walk(n, steps, drive=(1.0, 1.0), seed=5, **over):
    t = spec.tables()
    if over:
        t = spec.Tables(**{**t.__dict__, **over})
    st = spec.State(n, t, seed=seed)
    st.drive[:] = drive
    return t, st, st.advance(steps)


def test_the_settings_of_the_parity_runs():
    """16 bins over 24 steps: f takes non-zero values and a swing's steps come from a rounded-up quotient."""
    t = spec.tables()
    _, bins = swing_runs(_stance_of_the_fly())
    assert ((bins.astype(np.int64) * 24) % 16 != 0).any() and np.array_equal(t.swing_steps, -(-bins.astype(np.int64) * 24 // 16))
    assert (t.swing_steps >= 1).all() and (t.swing_steps < 24).all() and len(set(t.start_bin.tolist())) > 1
    assert spec.PARITY["seed"] != 0 and spec.PARITY["first_world"] != 0
    assert sum(spec.LAUNCHES) > 3 * 24 and set(spec.LAUNCHES) == {1, 31, 32, 33, 64}


def _stance_of_the_fly():
    from flygym_amd.controllers import TripodCPG
    from flygym_amd.models import make_model

    fly, world, _ = make_model()
    return TripodCPG(fly.get_actuated_jointdofs_order("position"), 1e-4, n_phase_bins=16).stance_bins(world.compile_model(), fly)


def test_stepping_the_specification():
    """40 worlds under the unit drive for 20 periods: no leg ever starts a step while its rule-1 source swings, every leg
    completes at least one step, counters stay in range, and every leg's first row is its rest pose."""
    n, P = 40, 24
    t, st, rows = _walk(n, 1)
    assert np.array_equal(rows[:, 0], np.broadcast_to(t.cycle[t.start_bin[t.leg_of_col], np.arange(42)], (n, 42)))
    assert st.stepping.sum(axis=1).tolist() == [1] * n and (st.ticks == 1).all()          # the fallback started one leg per world
    assert len(set(np.argmax(st.stepping, axis=1).tolist())) == 6                           # ... and not the same one everywhere
    completed = np.zeros((n, 6), dtype=int)
    for _ in range(20 * P - 1):
        before = st.counter.copy()
        st.advance(1)
        assert (st.counter >= 0).all() and (st.counter < P).all()
        assert ((st.counter == before) | (st.counter == (before + 1) % P)).all()
        assert np.array_equal(st.stepping != 0, st.counter != 0)
        completed += (before == P - 1) & (st.counter == 0)
    assert (completed >= 1).all(), completed.min(axis=0)
    assert len(st.starts) > 6 * n
    W1 = t.weights[0]
    for w, leg, k in st.starts:
        for src in np.nonzero(W1[:, leg])[0]:
            assert not 0 < k[src] < t.swing_steps[src], (w, leg, k)
    assert (st.ticks == 20 * P).all() and np.isfinite(st.scores).all()


def test_a_resting_leg_holds_its_rest_pose_whatever_the_amplitude():
    """No drive: nobody steps, and the row is the rest pose bit for bit at any amplitude; a foreign counter is reduced."""
    t = spec.tables(adhesion=spec.ADHESION)
    st = spec.State(3, t)
    st.drive[:] = 0
    st.amplitude[:] = np.array([0.0, 0.37, 1.5], dtype=np.float32)[:, None]
    rows = st.advance(30)
    rest = t.cycle[t.start_bin[t.leg_of_col], np.arange(42)]
    assert np.array_equal(rows[..., :42], np.broadcast_to(rest, (3, 30, 42))) and (rows[..., 42:] == 20.0).all()
    assert not st.counter.any() and not st.stepping.any() and (st.ticks == 30).all() and st.cover["none"] == 90
    st.counter[:] = np.array([-1, 24, 49, -25, 7, 23], dtype=np.int32)
    st.advance(1)
    assert st.counter.tolist() == [[23, 0, 1, 23, 7, 23]] * 3


def test_amplitude_is_latched_when_a_step_starts():
    """|drive| above max_amplitude is clamped, its sign is ignored, and a new drive does not touch a step under way."""
    t, st, _ = _walk(4, 1, drive=(-2.0, 0.5))
    leg = np.argmax(st.stepping, axis=1)
    want = np.where(leg < 3, np.float32(1.5), np.float32(0.5))
    assert np.array_equal(st.amplitude[np.arange(4), leg], want)
    others = np.ones((4, 6), dtype=bool)
    others[np.arange(4), leg] = False
    assert (st.amplitude[others] == 1).all()
    st.drive[:] = (0.25, 0.25)
    st.advance(3)
    assert np.array_equal(st.amplitude[np.arange(4), leg], want)


def test_the_parity_inputs_cover_what_the_kernel_can_get_wrong():
    """What ``tests/test_rules_gpu.py`` relies on, asserted on the specification alone."""
    for adhesion in (None, spec.ADHESION):
        _, cover, _ = spec.reference_run(23, adhesion)
        print(cover)
        assert cover["several"] >= 20, "fewer than 20 decisions with two or more eligible legs"
        assert {0, 1, 2} <= cover["picks"], f"a pick j out of 0, 1, 2 never occurs among them: {cover['picks']}"
        assert cover["single"] >= 20, "decisions with exactly one eligible leg are missing"
        assert cover["none"] >= 20, "decisions with no eligible leg are missing"
        assert cover["restarts"] >= 3, "the fallback is never taken at a tick other than 0 (the restart after a stop)"
        assert cover["completions"] >= 20, "no counter wraps to 0"
        assert cover["one_sided_starts"] >= 20, "no world has one side's drive at 0 while a leg of the other side starts"
        assert cover["clamped"] >= 20, "no latched amplitude is clamped by max_amplitude"
        assert cover["wrapped_rows"] >= 20, "no row has f != 0 with b1 wrapping to bin 0"
    for n in spec.CASES:                                   # every batch size sees starts, completions and a clamp
        _, cover, _ = spec.reference_run(n)
        assert cover["single"] >= 20 and cover["completions"] >= 20 and cover["clamped"] >= 1 and cover["wrapped_rows"] >= 20, (n, cover)
    drives = spec.input_run(23)
    stopped = (drives == 0).all(axis=2)                    # (launches, worlds)
    steps = np.array(spec.LAUNCHES)
    assert any(steps[stopped[:, w]].sum() > 24 and not stopped[-1, w] for w in range(23))
    assert ((drives[:, :, 0] == 0) & (drives[:, :, 1] != 0)).all(axis=0).any() and (drives > 1.5).any()
    assert any(len(set(drives[:, w, 0].tolist())) > 1 for w in range(23)) and drives.flags.writeable is False
