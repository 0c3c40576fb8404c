"""The walking task's specification (``tests/task_spec.py``) on its own, and what of ``flygym_amd.tasks`` needs no device: that the
inputs the GPU parity tests use reach every branch of the rule, that the power sum does not depend on the order of the actuators,
one small case against numbers written out by hand, what a bad world gets, and the argument errors of ``WalkingTask`` / ``TaskEnv``."""
import ctypes

import numpy as np
import pytest

import task_spec as spec

f32 = np.float32


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("n_act,n_q", spec.COMBOS)
@pytest.mark.parametrize("n,T", spec.CASES)
def test_the_parity_inputs_reach_every_branch(n, T, n_act, n_q, shared):
    """Every reason bit, truncation, the grace period suppressing a reason, a tilt and an airborne counter that reach their limit
    and ones that are cut short, GOAL, the fresh tick and a nonzero progress each occur in at least three (update, world) pairs of
    every case the GPU test runs; planted values include NaN, +-Inf and denormals in every input array."""
    snaps, cover = spec.reference_run(n, T, n_act, n_q, shared)
    assert set(cover) >= {*spec.REASONS, "truncated", "grace_suppressed", "tilt_limit", "tilt_cut_short", "airborne_limit",
                          "airborne_cut_short", "fresh", "progress"}
    assert min(cover.values()) >= 3, cover
    assert 60 <= T <= 120 and len(snaps) == T
    for s in snaps:                                                       # whatever the inputs were, the accounts stay finite
        assert all(np.isfinite(s[name]).all() for name in ("reward", "obs", "ep_return", "last_return", "prev_xy"))
    if n == 257:                                                          # every input array gets every planted kind somewhere
        run = spec.input_run(n, T, n_act, n_q)
        for name in spec.INPUTS:
            a = run[name]
            assert np.isnan(a).any() and np.isposinf(a).any() and np.isneginf(a).any(), name
            assert ((a != 0) & (np.abs(a) < np.finfo(f32).tiny)).any(), name


def test_the_last_world_is_the_same_world_in_every_batch():
    for n_act, n_q in spec.COMBOS:
        runs = [(spec.input_run(n, T, n_act, n_q), T) for n, T in spec.CASES]
        for name in (*spec.INPUTS, "course", "goal"):
            for other, T in runs[1:]:
                a, b = (runs[0][0][name][:T, 0], other[name][:, -1]) if name in spec.INPUTS else (runs[0][0][name][0], other[name][-1])
                assert a.tobytes() == b.tobytes(), name


def test_the_power_sum_does_not_depend_on_the_order_of_the_actuators():
    rng = np.random.default_rng(1)
    force = (rng.normal(0, 30, (200, 42)) * 10.0 ** rng.integers(-3, 3, (200, 42))).astype(f32)
    qd = rng.normal(0, 10, (200, 42)).astype(f32)
    force[3, 5], qd[7, 1], force[9, 9] = np.nan, np.inf, 1e-41
    P0, power0 = spec.power_sum(force, qd, f32(50.0))
    for _ in range(5):
        perm = rng.permutation(42)
        P1, power1 = spec.power_sum(force[:, perm], qd[:, perm], f32(50.0))
        assert np.array_equal(P0, P1) and power0.tobytes() == power1.tobytes()
    assert P0.dtype == np.int32 and 0 < P0.max() <= 42 * 50 * 1024 and np.isfinite(power0).all()
    # a float32 sum of the same terms does depend on it: that is why the sum is an integer one
    terms = np.minimum(np.abs(np.nan_to_num(force * qd, posinf=0)), f32(50))
    sums = {np.add.reduce(terms[:, rng.permutation(42)], axis=1, dtype=f32).tobytes() for _ in range(8)}
    assert len(sums) > 1


def test_two_worlds_three_ticks_by_hand():
    """Two worlds, three ticks, every number written out (one actuator, one observed dof, upright and level), then two more
    ticks with one world on its side and the other too high."""
    p = spec.Params(tilt_ticks=2, airborne_ticks=2, max_ticks=3, grace_ticks=1, cos_max_tilt=0.5, z_min=0.5, z_max=2.0,
                    arena=(-10, 10, -10, 10), goal_radius2=0.25, power_clip=4.0, thr2=(1, 1, 1, 1, 1, 1), alive=0.5, w_progress=2.0,
                    w_power=0.25, w_tilt=1.0, bonus_goal=10.0, penalty_fail=3.0)
    st = spec.State(2, p, 1, mean=[0.5], inv_std=[2.0])
    st.course[:] = [[1, 0], [0, 1]]
    st.goal[:] = [[3, 0], [100, 100]]
    quat = np.array([[1, 0, 0, 0], [1, 0, 0, 0]], dtype=f32)
    stand = np.zeros((2, 6, 4), dtype=f32)
    stand[:, 0] = (1, 0, 0, 2)                                            # the first leg touches with |F|^2 = 4 > 1
    vel = np.array([[1, 2, 3, 4, 5, 6], [0, 0, 0, 0, 0, 0]], dtype=f32)
    ang = np.array([[1.0], [0.5]], dtype=f32)
    # tick 1: fresh, so no progress; power = |2 * 1.5| = 3 and |8 * 1| clipped to 4
    st.update([[1, 0, 1], [0, 0, 1]], quat, vel, [[2.0], [8.0]], [[1.5], [1.0]], stand, ang)
    assert st.reward.tolist() == [0.5 - 0.25 * 3, 0.5 - 0.25 * 4] and st.done.tolist() == [0, 0] and st.fresh.tolist() == [0, 0]
    assert st.obs[0].tolist() == [0, 0, -1, 1, 2, 3, 4, 5, 6, 2, 0, 1, 1, 0, 0, 0, 0, 0, 1.0]
    assert st.obs[1].tolist() == [0, 0, -1, 0, 0, 0, 0, 0, 0, 100, 100, 1, 1, 0, 0, 0, 0, 0, 0.0]
    # tick 2: world 0 moves 1.75 along its course into the goal disc (distance 0.25): +2 * 1.75 + 10; world 1 moves 0.5 along y
    # and lifts every leg: airborne_count 1
    air = np.zeros((2, 6, 4), dtype=f32)
    st.update([[2.75, 0, 1], [7, 0.5, 1]], quat, vel, [[0.0], [0.0]], [[0.0], [0.0]], np.stack([stand[0], air[1]]), ang)
    assert st.reward.tolist() == [0.5 + 3.5 + 10, 0.5 + 1.0] and st.reason.tolist() == [spec.GOAL, 0]
    assert st.terminated.tolist() == [1, 0] and st.done.tolist() == [1, 0] and st.fresh.tolist() == [1, 0]
    assert st.last_return.tolist() == [-0.25 + 14.0, 0] and st.last_length.tolist() == [2, 0] and st.successes.tolist() == [1, 0]
    assert st.ep_return.tolist() == [0, 1.0] and st.ep_length.tolist() == [0, 2] and st.airborne_count.tolist() == [0, 1]
    assert st.prev_xy.tolist() == [[0, 0], [7, 0.5]]
    # tick 3: world 0 starts afresh (no progress, though it moved); world 1 is still airborne: count 2 = the limit, -3, and it is
    # also at its time limit, which a termination hides
    st.update([[5, 5, 1], [7, 0.5, 1]], quat, vel, [[0.0], [0.0]], [[0.0], [0.0]], np.stack([stand[0], air[1]]), ang)
    assert st.reward.tolist() == [0.5, 0.5 - 3.0] and st.reason.tolist() == [0, spec.AIRBORNE] and st.truncated.tolist() == [0, 0]
    assert st.episodes.tolist() == [1, 1] and st.last_reason.tolist() == [spec.GOAL, spec.AIRBORNE] and st.last_return.tolist() == [13.75, -1.5]
    assert st.ep_length.tolist() == [1, 0] and st.fresh.tolist() == [0, 1]
    # a tilt of 90 degrees about x: up_z = 0, gravity along -y of the body, w_tilt * 1 off the reward; the first tick is in grace
    s = f32(np.sqrt(0.5))
    st.update([[5, 5, 1], [0, 0, 9]], [[s, s, 0, 0], [1, 0, 0, 0]], vel, [[0.0], [0.0]], [[0.0], [0.0]], stand, ang)
    assert abs(st.reward[0] - (0.5 - 1.0)) < 1e-6 and st.tilt_count.tolist() == [1, 0] and st.reason.tolist() == [0, 0]
    assert np.allclose(st.obs[0, :3], [0, -1, 0], atol=1e-6) and np.allclose(st.obs[0, 3:6], [1, 3, -2], atol=1e-6)
    st.update([[5, 5, 1], [0, 0, 9]], [[s, s, 0, 0], [1, 0, 0, 0]], vel, [[0.0], [0.0]], [[0.0], [0.0]], stand, ang)
    assert st.reason.tolist() == [spec.TILTED, spec.HEIGHT]               # tilt_count 2 = the limit; z = 9 out of grace


def test_a_bad_world():
    """A NaN, an Inf anywhere in what a world reads: reward exactly -penalty_fail, a row of zeros, NONFINITE alone, finite accounts."""
    n_act, n_q = 17, 3
    run = spec.input_run(5, 100, n_act, n_q)
    p = spec.PARITY
    for name in spec.INPUTS:
        for value in (np.nan, np.inf, -np.inf):
            st = spec.State(5, p, n_q, *spec.standardisation(n_q))
            st.goal[:] = run["goal"]
            inputs = {k: run[k][0].copy() for k in spec.INPUTS}
            st.update(*(inputs[k] for k in spec.INPUTS))
            inputs = {k: run[k][1].copy() for k in spec.INPUTS}
            inputs[name].reshape(5, -1)[2, -1] = value
            before = st.ep_return.copy()
            st.update(*(inputs[k] for k in spec.INPUTS))
            assert st.reward[2].tobytes() == f32(-p.penalty_fail).tobytes() and not st.obs[2].any() and st.reason[2] == spec.NONFINITE
            assert st.terminated[2] == 1 and st.done[2] == 1 and st.last_return[2] == before[2] - p.penalty_fail
            assert all(np.isfinite(getattr(st, k)).all() for k in ("reward", "obs", "ep_return", "last_return", "prev_xy"))
            assert st.ep_return[2] == 0 and st.fresh[2] == 1 and (st.prev_xy[2] == 0).all()
    st = spec.State(1, p, 1)
    st.course[0, 1] = np.nan                                              # the handle's own arrays count too
    st.update([[0, 0, 1]], [[1, 0, 0, 0]], np.zeros((1, 6)), [[0]], [[0]], np.zeros((1, 6, 4)), [[0]])
    assert st.reason[0] == spec.NONFINITE and st.reward[0] == -p.penalty_fail
    # a denormal is an ordinary number
    st = spec.State(1, p, 1)
    st.goal[:] = 5
    st.update([[0, 0, 1]], [[1, 0, 0, 0]], np.full((1, 6), 1e-40, dtype=f32), [[0]], [[0]], np.zeros((1, 6, 4)), [[1e-41]])
    assert st.reason[0] == 0 and st.obs[0, 3] == f32(1e-40) and st.obs[0, 18] == f32(1e-41)


def test_the_params_mirror_and_argument_errors():
    """The ctypes mirror has the layout of ``nmf_task_params`` (4-byte members only); ``TaskEnv`` and ``WalkingTask`` refuse what
    they can see without a device."""
    from flygym_amd.tasks import REASONS, TaskEnv, WalkingTask, _TaskParams

    assert ctypes.sizeof(_TaskParams) == 4 * (7 + 3 + 4 + 2 + 6 + 6) and REASONS == spec.REASONS
    assert [name for name, _ in _TaskParams._fields_ if name in spec.Params.__dataclass_fields__] != []
    assert set(spec.Params.__dataclass_fields__) == {name for name, _ in _TaskParams._fields_} - {"root_seg", "n_act", "n_q"}
    assert WalkingTask._views == spec.FIELDS
    import flygym_amd

    assert flygym_amd.WalkingTask is WalkingTask and flygym_amd.TaskEnv is TaskEnv

    class Several:
        for_fly = None

    with pytest.raises(ValueError, match="for_fly"):
        WalkingTask(Several(), "nmf")

    class Sim:
        n_worlds = 4

        class world:
            fly_lookup = {}

    with pytest.raises(ValueError, match="no fly named"):
        WalkingTask(Sim(), "nmf")

    class Controller:
        drive = None

        def step(self, n): ...

        def reset(self, mask=None): ...

    with pytest.raises(TypeError, match="has no .drive"):
        TaskEnv(Sim(), object(), None)
    with pytest.raises(TypeError, match="has no .reset"):
        TaskEnv(Sim(), type("C", (), dict(drive=None, step=None))(), None)
    with pytest.raises(TypeError, match="WalkingTask"):
        TaskEnv(Sim(), Controller(), object())
    task = WalkingTask.__new__(WalkingTask)                               # (no handle: enough for the checks before the device)
    task.sim, task.n_worlds = Sim(), 4
    for name in WalkingTask._views:
        setattr(task, name, None)
    sim = task.sim
    with pytest.raises(ValueError, match="another batch"):
        TaskEnv(Sim(), Controller(), task)
    other = Controller()
    other.sim = Sim()
    with pytest.raises(ValueError, match="controller belongs"):
        TaskEnv(sim, other, task)
    with pytest.raises(ValueError, match="steps_per_tick"):
        TaskEnv(sim, Controller(), task, steps_per_tick=0)
    with pytest.raises(TypeError, match="also_reset"):
        TaskEnv(sim, Controller(), task, also_reset=(object(),))
    with pytest.raises(RuntimeError, match="the task is closed"):
        task.update()
    with pytest.raises(RuntimeError, match="the task is closed"):
        task.reset()
