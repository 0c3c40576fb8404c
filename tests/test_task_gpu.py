"""The walking task on the GPU (``flygym_amd/csrc/nmf_task.hip``, ``flygym_amd.tasks.WalkingTask`` / ``TaskEnv``) against its numpy
specification ``tests/task_spec.py``.

The inputs are synthetic except in the captured-graph, ``TaskEnv`` and real-physics tests: after ``sim.reset()`` the tests write
chosen root poses, velocities, forces, sensor blocks and joint angles into the zero-copy views of the batch; nothing steps in
between, so the inputs are exactly known.  The comparison rule: every view equals the specification's bytes after every update.
``tests/test_task_cpu.py`` asserts that the inputs used here reach every reason, truncation, the grace period and the counters."""
import ctypes
import functools

import numpy as np
import pytest

import task_spec as spec

pytestmark = pytest.mark.gpu

FIELDS = spec.FIELDS
KEYS = ("qpos", "qvel", "ctrl", "seg_xpos", "seg_xquat", "sensordata", "time")
P = spec.PARITY
PARITY_KW = dict(contact_force_thr=(0.5, 1.0, 3.0), max_tilt=60.0, tilt_ticks=P.tilt_ticks, airborne_ticks=P.airborne_ticks,
                 grace_ticks=P.grace_ticks, max_ticks=P.max_ticks, z_range=(0.5, 2.5), arena=(-10.0, 10.0, -10.0, 10.0), goal_radius=1.0,
                 power_clip=50.0, alive=0.1, w_progress=2.0, w_power=0.01, w_tilt=0.5, bonus_goal=10.0, penalty_fail=5.0)


@pytest.fixture
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch


@functools.lru_cache(maxsize=None)
def _batch(n, copy=0):
    from flygym_amd import HIPSimulation, make_model

    fly, world, _ = make_model()
    sim = HIPSimulation(world, n_worlds=n, device=0)
    sim.set_leg_adhesion_states(fly.name, np.ones((n, 6), dtype=np.float32))
    sim.reset()
    return sim, fly


def _task(sim, fly, n_act=42, n_q=42, **over):
    """A task with the parity settings of the specification module (``spec.PARITY``): the first ``n_act`` / ``n_q`` leg dofs."""
    from flygym_amd.anatomy import LEGS
    from flygym_amd.tasks import WalkingTask

    dofs = [d for d in fly.get_actuated_jointdofs_order("position") if d.child.pos in LEGS]
    mean, inv_std = spec.standardisation(n_q)
    kw = dict(actuators=dofs[:n_act], obs_dofs=dofs[:n_q], obs_mean=mean, obs_std=(1.0 / inv_std.astype(np.float64)), **PARITY_KW)
    task = WalkingTask(sim, fly.name, **{**kw, **over})
    if "obs_std" not in over and "obs_dofs" not in over:
        assert np.array_equal(task._inv_std, inv_std)                     # (1 / (1 / x) in float64 rounds back to x)
    return task


class _Inputs:
    """Where a task's inputs live in the batch: writes one update's inputs into the views, reads them back."""

    def __init__(self, torch, sim, task):
        n, nseg = sim.n_worlds, sim.model.nseg
        ids = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int64), device=sim.device)
        self.torch, self.act, self.act_dof, self.obs_dof = torch, ids(task._act), ids(6 + task._act_dof), ids(7 + task._obs_dof)
        self.pos = sim.field("seg_xpos").view(n, nseg, 3)[:, task.root_seg]
        self.quat = sim.field("seg_xquat").view(n, nseg, 4)[:, task.root_seg]
        self.qvel, self.qpos, self.force = sim.field("qvel"), sim.field("qpos"), sim.field("actuator_force")
        self.sens = sim.field("sensordata").view(n, 6, 16)

    def write(self, run, k):
        self.pos.copy_(run["pos"][k]); self.quat.copy_(run["quat"][k])
        self.qvel[:, :6] = run["vel"][k]
        self.qvel[:, self.act_dof] = run["qd"][k]
        self.force[:, self.act] = run["force"][k]
        self.sens[:, :, :4] = run["sens"][k]
        self.qpos[:, self.obs_dof] = run["ang"][k]

    def read(self):
        """What an update would read now, as numpy in the order of ``spec.INPUTS``."""
        parts = (self.pos, self.quat, self.qvel[:, :6], self.force[:, self.act], self.qvel[:, self.act_dof], self.sens[:, :, :4],
                 self.qpos[:, self.obs_dof])
        parts = [a.clone() for a in parts]
        self.torch.cuda.synchronize()
        return [a.cpu().numpy() for a in parts]


def _clone(task):
    return {name: getattr(task, name).clone() for name in FIELDS}


def _numpy(torch, clones):
    """A list of per-update dicts of device tensors -> one dict of stacked numpy arrays (T, n, ...)."""
    torch.cuda.synchronize()
    return {name: torch.stack([c[name] for c in clones]).cpu().numpy() for name in FIELDS}


def _stacked(snaps):
    return {name: np.stack([s[name] for s in snaps]) for name in FIELDS}


def _assert_same(got, want, where, worlds=slice(None)):
    for name in FIELDS:
        g, w = got[name][:, worlds], want[name][:, worlds]
        assert g.dtype == w.dtype and g.shape == w.shape, (where, name, g.dtype, w.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            gb, wb = (np.ascontiguousarray(a).view(np.uint8).reshape(*a.shape, -1) for a in (g, w))
            first = [tuple(i) for i in np.argwhere((gb != wb).any(axis=-1))[:3]]
            raise AssertionError((where, name, "first differences at (update, world, ...)", first, [(g[i], w[i]) for i in first]))


def _device_run(torch, run):
    return {name: torch.as_tensor(np.array(a), device="cuda:0") for name, a in run.items()}


@functools.lru_cache(maxsize=None)
def _gpu_run(n, T, n_act, n_q, layout):
    """T updates of an n-world batch on the device from the specification module's inputs; every view after every update, as numpy.
    layout: "rows" one course row per world; "shared" the course of world n - 1 set as one shared row; "repeated" that row n times."""
    import torch

    sim, fly = _batch(n)
    sim.reset()
    run = _device_run(torch, spec.input_run(n, T, n_act, n_q))
    clones = []
    with _task(sim, fly, n_act, n_q) as task:
        assert spec.Params.from_struct(task._params) == P and (task.n_act, task.n_q, task.obs_width) == (n_act, n_q, 18 + n_q)
        assert tuple(task.obs.shape) == (n, 18 + n_q) and tuple(task.reward.shape) == (n,) and tuple(task.course.shape) == (n, 2)
        assert task.done.dtype == torch.uint8 and task.reason.dtype == torch.int32 and bool(task.fresh.all())
        assert torch.equal(task.course, torch.tensor([[1.0, 0.0]], device=sim.device).expand(n, 2)) and not bool(task.goal.any())
        if layout == "rows":
            task.course.copy_(run["course"])
        elif layout == "shared":
            task.set_course(run["course"][-1], normalise=False)          # (exact values)
            task.set_goal(run["goal"])
        else:
            task.course.copy_(run["course"][-1:].expand(n, 2).contiguous())
        task.goal.copy_(run["goal"])
        io = _Inputs(torch, sim, task)
        for k in range(T):
            io.write(run, k)
            out = task.update()
            assert out[0] is task.obs and out[1] is task.reward and out[2] is task.terminated and out[3] is task.truncated
            clones.append(_clone(task))
        got = _numpy(torch, clones)
    for a in got.values():
        a.setflags(write=False)
    return got


@pytest.mark.parametrize("layout", ["rows", "shared", "repeated"])
@pytest.mark.parametrize("n_act,n_q", spec.COMBOS)
@pytest.mark.parametrize("n,T", spec.CASES)
def test_parity_with_the_specification(torch_mod, n, T, n_act, n_q, layout):
    """1, 5, 17 and 257 worlds (one world, one past a wave's four, one past a workgroup's sixteen, many workgroups), 120 to 60
    updates, (n_act, n_q) = (1, 1), (17, 3), (42, 42): random and scripted poses, velocities, forces, sensor blocks and angles with
    NaN, +-Inf and denormals among them; every view after every update equals the specification's bytes.  One course row per
    world, one shared row, and that row repeated: the last two give identical results."""
    snaps, cover = spec.reference_run(n, T, n_act, n_q, layout != "rows")
    got = _gpu_run(n, T, n_act, n_q, layout)
    _assert_same(got, _stacked(snaps), (n, T, n_act, n_q, layout))
    if layout == "repeated":
        shared = _gpu_run(n, T, n_act, n_q, "shared")
        assert all(got[name].tobytes() == shared[name].tobytes() for name in FIELDS)
    assert min(cover.values()) >= 3
    print(f"task parity, {n} worlds x {T} updates, n_act {n_act}, n_q {n_q}, course {layout}: all views bit for bit; {cover}")


@pytest.mark.parametrize("n_act,n_q", spec.COMBOS)
def test_a_world_does_not_depend_on_its_place_in_the_batch(torch_mod, n_act, n_q):
    """World n - 1 of the 1-, 5-, 17- and 257-world batches gets the same inputs, course and goal: it is byte-identical after
    every one of the updates the runs share."""
    runs = [(_gpu_run(n, T, n_act, n_q, "shared"), T) for n, T in spec.CASES]
    for name in FIELDS:
        for other, T in runs[1:]:
            assert runs[0][0][name][:T, 0].tobytes() == other[name][:, -1].tobytes(), name
    alone = runs[0][0]
    assert alone["episodes"][-1, 0] >= 21 and len(np.unique(alone["last_reason"][:, 0])) >= 7


def test_masked_reset(torch_mod):
    """17 worlds; after 20 updates the odd ones are reset and everything runs 25 more.  The masked worlds start a fresh episode with
    empty statistics and follow a specification reset the same way; the others are byte-identical to an undisturbed twin."""
    torch = torch_mod
    n, T0, T1, n_act, n_q = 17, 20, 25, 17, 3
    sim, fly = _batch(n)
    sim.reset()
    host = spec.input_run(n, T0 + T1, n_act, n_q)
    run = _device_run(torch, host)
    mask = np.arange(n) % 2 == 1
    st = spec.State(n, P, n_q, *spec.standardisation(n_q))
    st.course[:], st.goal[:] = host["course"], host["goal"]
    snaps = []
    with _task(sim, fly, n_act, n_q) as task, _task(sim, fly, n_act, n_q) as twin:
        for t in (task, twin):
            t.course.copy_(run["course"]); t.goal.copy_(run["goal"])
        io = _Inputs(torch, sim, task)
        clones, twins = [], []

        def go(k0, k1):
            for k in range(k0, k1):
                io.write(run, k)
                task.update(); twin.update()
                clones.append(_clone(task)); twins.append(_clone(twin))
                st.update(*(host[name][k] for name in spec.INPUTS))
                snaps.append(st.snapshot())

        go(0, T0)
        before = _numpy(torch, clones[-1:])
        assert before["episodes"][0, mask].any() and before["last_return"][0, mask].any() and before["obs"][0, mask].any()
        task.reset(torch.as_tensor(mask))
        st.reset(mask)
        after = _numpy(torch, [_clone(task)])
        for name in FIELDS:
            if name in ("course", "goal"):
                assert after[name].tobytes() == before[name].tobytes(), name
                continue
            assert (after[name][0, mask] == (1 if name == "fresh" else 0)).all(), name
            assert after[name][0, ~mask].tobytes() == before[name][0, ~mask].tobytes(), name
        go(T0, T0 + T1)
        got, undisturbed = _numpy(torch, clones), _numpy(torch, twins)
        _assert_same(got, _stacked(snaps), "masked reset")
        for name in FIELDS:
            assert got[name][:, ~mask].tobytes() == undisturbed[name][:, ~mask].tobytes(), name
        assert got["episodes"][T0:, mask].tobytes() != undisturbed["episodes"][T0:, mask].tobytes()
        task.reset(np.ones(n, dtype=bool)); twin.reset()
        both = _numpy(torch, [_clone(task), _clone(twin)])
        assert all((both[name] == (1 if name == "fresh" else 0)).all() for name in FIELDS if name not in ("course", "goal"))


def _settled(torch, n, copy, **task_kw):
    from flygym_amd.controllers import TurningCPG

    sim, fly = _batch(n, copy=copy)
    sim.reset()
    sim.warmup()
    cpg = TurningCPG(sim, fly.name, table_steps=32)
    cpg.step(20)                                                                   # every kernel of the chain has run once
    task = _task(sim, fly, **task_kw)
    return sim, fly, cpg, task


def test_one_control_tick_is_one_captured_graph(torch_mod):
    """Two settled 11-world batches.  One tick is ``cpg.step(20)``, ``task.update()``, ``sim.reset_worlds(task.done)``,
    ``cpg.reset(task.done)``: twelve eager ticks on one batch against one capture replayed twelve times on the other (one stream, one
    linear chain).  A time limit of 5 ticks and goal discs around three worlds' start points end episodes in every world; all task
    views and the batch fields are identical tick by tick, and the specification, fed the inputs recorded before each eager update,
    agrees bit for bit."""
    torch = torch_mod
    n, ticks, steps = 11, 12, 20
    kw = dict(max_ticks=5, grace_ticks=0, goal_radius=0.6, z_range=(-10.0, 10.0), max_tilt=179.0, airborne_ticks=1000, power_clip=4096.0)
    (s0, _, c0, t0), (s1, _, c1, t1) = (_settled(torch, n, copy, **kw) for copy in (1, 2))
    io = _Inputs(torch, s0, t0)
    goal = torch.full((n, 2), 100.0, device=s0.device)
    goal[2:5] = io.pos[2:5, :2] + 0.2                                              # three worlds stand inside their goal disc
    for t in (t0, t1):
        t.set_goal(goal)
        t.set_course((0.6, 0.8))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c1.step(steps)
        t1.update()
        s1.reset_worlds(t1.done)
        c1.reset(t1.done)
    assert not bool(t1.ep_length.any()) and not bool(t1.episodes.any())            # (the capture itself ran nothing)
    st = spec.State(n, spec.Params.from_struct(t0._params), 42, *spec.standardisation(42))
    st.course[:], st.goal[:] = t0.course.cpu().numpy(), t0.goal.cpu().numpy()
    resets = np.zeros(n, dtype=np.int64)
    for k in range(ticks):
        c0.step(steps)
        recorded = io.read()
        t0.update()
        eager = _numpy(torch, [_clone(t0)])
        s0.reset_worlds(t0.done)
        c0.reset(t0.done)
        g.replay()
        st.update(*recorded)
        resets += st.done
        replayed = _numpy(torch, [_clone(t1)])
        _assert_same(eager, _stacked([st.snapshot()]), ("tick", k))
        for name in FIELDS:
            assert eager[name].tobytes() == replayed[name].tobytes(), (k, name)
        for key in KEYS:
            assert torch.equal(s0.field(key), s1.field(key)), (k, key)
    print(f"task in the captured tick, {n} worlds x {ticks} ticks: resets per world {resets.tolist()}, goals {int(st.successes.sum())}, "
          f"reasons now {st.last_reason.tolist()}")
    assert int((resets > 0).sum()) >= 3 and int(st.successes.sum()) >= 3 and int((st.last_reason == 0).sum()) >= 3
    assert not (st.last_reason & spec.NONFINITE).any()
    for c, t in ((c0, t0), (c1, t1)):
        t.close(); c.close()


def test_task_env_captured_against_eager(torch_mod):
    """Twin settled 11-world batches, the same ten actions: ``TaskEnv(capture=True)`` returns what ``TaskEnv(capture=False)``
    returns, tick by tick; the returned objects are the task's views, and ``info["episodes"]`` grows."""
    torch = torch_mod
    from flygym_amd.tasks import TaskEnv

    n, ticks = 11, 10
    kw = dict(max_ticks=4, grace_ticks=0, goal_radius=0.0, z_range=(-10.0, 10.0), max_tilt=179.0, airborne_ticks=1000, power_clip=4096.0)
    sides = [_settled(torch, n, copy, **kw) for copy in (1, 2)]
    envs = [TaskEnv(sim, cpg, task, steps_per_tick=20, capture=capture) for (sim, _, cpg, task), capture in zip(sides, (False, True))]
    rng = np.random.default_rng(4)
    actions = torch.as_tensor(rng.uniform(0.4, 1.2, (ticks, n, 2)).astype(np.float32), device=sides[0][0].device)
    for k in range(ticks):
        outs = [env.step(actions[k]) for env in envs]
        for env, out in zip(envs, outs):
            assert out[0] is env.task.obs and out[1] is env.task.reward and out[2] is env.task.terminated and out[3] is env.task.truncated
            assert out[4]["episodes"] is env.task.episodes and out[4]["reason"] is env.task.reason
            assert set(out[4]) == {"reason", "episodes", "last_return", "last_length"}
        torch.cuda.synchronize()
        for a, b in zip(outs[0][:4], outs[1][:4]):
            assert torch.equal(a, b), k
        for name in FIELDS:
            assert torch.equal(getattr(envs[0].task, name), getattr(envs[1].task, name)), (k, name)
        for key in KEYS:
            assert torch.equal(sides[0][0].field(key), sides[1][0].field(key)), (k, key)
    assert envs[1]._graph is not None and envs[0]._graph is None
    assert int(envs[1].info["episodes"].sum()) == 2 * n and bool(outs[1][1].isfinite().all())
    first = [env.reset() for env in envs]
    assert first[0] is envs[0].task.obs and torch.equal(first[0], first[1]) and int(envs[1].task.ep_length.max()) == 1
    with pytest.raises(ValueError, match="action"):
        envs[0].step(actions[0][:, :1])
    with pytest.raises(ValueError, match="action"):
        envs[0].step(actions[0].cpu())
    for _, _, cpg, task in sides:
        task.close(); cpg.close()


def test_refusals_leave_the_state_untouched(torch_mod):
    """Every refused creation, at the C ABI and through the class, names its cause and leaks nothing (a following valid creation
    works); a live task's views read the same before and after each refusal; a closed task refuses update and reset; a world with
    several flies asks for ``for_fly``."""
    torch = torch_mod
    from flygym_amd import _native
    from flygym_amd.tasks import WalkingTask, _TaskParams

    lib = _native.lib()
    n, n_act, n_q = 5, 17, 3
    sim, fly = _batch(n)
    sim.reset()
    run = _device_run(torch, spec.input_run(n, 12, n_act, n_q))
    live = _task(sim, fly, n_act, n_q)
    live.goal.copy_(run["goal"])
    io = _Inputs(torch, sim, live)
    for k in range(12):
        io.write(run, k)
        live.update()
    before = _numpy(torch, [_clone(live)])
    assert before["obs"].any() and before["episodes"].any() and before["last_return"].any()

    def unchanged():
        now = _numpy(torch, [_clone(live)])
        assert all(now[name].tobytes() == before[name].tobytes() for name in FIELDS)

    arrays = dict(act=live._act.copy(), act_dof=live._act_dof.copy(), obs_dof=live._obs_dof.copy(), mean=live._mean.copy(),
                  inv_std=live._inv_std.copy())

    def create(arr=None, **over):
        p = _TaskParams.from_buffer_copy(live._params)
        for key, value in over.items():
            if isinstance(value, tuple):
                getattr(p, key)[value[0]] = value[1]
            else:
                setattr(p, key, value)
        a = {k: v.copy() for k, v in arrays.items()}
        for key, value in (arr or {}).items():
            if key != "null":
                a[key][value[0]] = value[1]
        ptrs = [None if (arr or {}).get("null") == k else a[k].ctypes.data for k in ("act", "act_dof", "obs_dof", "mean", "inv_std")]
        return lib.nmf_task_create(sim._batch_h, ctypes.byref(p), *ptrs)

    nan, inf = float("nan"), float("inf")
    nseg, nu, n_dof = sim.model.nseg, sim.model.nu, sim.model.nq - 7
    refusals = [(dict(cos_max_tilt=nan), {}, b"not finite"), (dict(z_max=inf), {}, b"not finite"), (dict(arena=(2, -inf)), {}, b"not finite"),
                (dict(goal_radius2=nan), {}, b"not finite"), (dict(power_clip=inf), {}, b"not finite"), (dict(thr2=(4, nan)), {}, b"not finite"),
                (dict(alive=nan), {}, b"not finite"), (dict(w_progress=inf), {}, b"not finite"), (dict(w_power=nan), {}, b"not finite"),
                (dict(w_tilt=-inf), {}, b"not finite"), (dict(bonus_goal=nan), {}, b"not finite"), (dict(penalty_fail=inf), {}, b"not finite"),
                ({}, dict(mean=(1, nan)), b"mean or inv_std"), ({}, dict(inv_std=(0, inf)), b"mean or inv_std"),
                (dict(root_seg=nseg), {}, b"root_seg"), (dict(root_seg=-1), {}, b"root_seg"),
                ({}, dict(act=(3, nu)), b"act[3]"), ({}, dict(act=(0, -1)), b"act[0]"), ({}, dict(act_dof=(16, n_dof)), b"act_dof[16]"),
                ({}, dict(act_dof=(2, -1)), b"act_dof[2]"), ({}, dict(obs_dof=(2, n_dof)), b"obs_dof[2]"), ({}, dict(obs_dof=(0, -5)), b"obs_dof[0]"),
                (dict(n_act=65), {}, b"n_act"), (dict(n_act=0), {}, b"n_act"), (dict(n_q=257), {}, b"n_q"), (dict(n_q=0), {}, b"n_q"),
                (dict(tilt_ticks=0), {}, b"tilt_ticks"), (dict(airborne_ticks=0), {}, b"airborne_ticks"), (dict(max_ticks=0), {}, b"max_ticks"),
                (dict(grace_ticks=-1), {}, b"grace_ticks"), (dict(cos_max_tilt=1.5), {}, b"cos_max_tilt"),
                (dict(z_min=3.0, z_max=1.0), {}, b"z_min > z_max"), (dict(arena=(1, -10.0)), {}, b"arena is empty"),
                (dict(arena=(2, 10.0)), {}, b"arena is empty"), (dict(goal_radius2=-1.0), {}, b"goal_radius2"), (dict(thr2=(5, -1.0)), {}, b"thr2"),
                (dict(power_clip=-1.0), {}, b"power_clip"), (dict(power_clip=2.0 ** 21), {}, b"power_clip"),
                ({}, dict(null="act"), b"null"), ({}, dict(null="act_dof"), b"null"), ({}, dict(null="obs_dof"), b"null"),
                ({}, dict(null="mean"), b"null"), ({}, dict(null="inv_std"), b"null")]
    for over, arr, text in refusals:
        assert not create(arr, **over) and text in lib.nmf_last_error(), (over, arr, lib.nmf_last_error())
        unchanged()
    ok = [arrays[k].ctypes.data for k in ("act", "act_dof", "obs_dof", "mean", "inv_std")]
    assert not lib.nmf_task_create(sim._batch_h, None, *ok) and b"null" in lib.nmf_last_error()
    assert not lib.nmf_task_create(None, ctypes.byref(live._params), *ok) and b"null" in lib.nmf_last_error()
    assert 17 * round(2.0 ** 21 * 1024) > 2 ** 31 - 1 >= 17 * round(50.0 * 1024)      # (why that power_clip is refused)
    # the Python class raises NativeError with the library's message, or ValueError before it gets there
    for over, text in ((dict(z_range=(3.0, 1.0)), "z_min > z_max"), (dict(arena=(5.0, 5.0, -1.0, 1.0)), "arena is empty"),
                       (dict(tilt_ticks=0), "tilt_ticks must be at least 1"), (dict(power_clip=1e9), "power_clip must be in"),
                       (dict(w_tilt=nan), "not finite"), (dict(grace_ticks=-3), "grace_ticks")):
        with pytest.raises(_native.NativeError, match=text):
            _task(sim, fly, n_act, n_q, **over)
    for over, text in ((dict(obs_std=np.zeros(n_q)), "obs_std"), (dict(obs_mean=np.zeros(n_q + 1)), "obs_mean"), (dict(max_tilt=200.0), "max_tilt"),
                       (dict(goal_radius=-1.0), "goal_radius"), (dict(actuators=["no-such-dof"]), "no position actuator"),
                       (dict(obs_dofs=["no-such-dof"]), "no joint dof"), (dict(contact_force_thr=(1.0, 2.0)), "contact_force_thr"),
                       (dict(actuators=[]), "actuators takes")):
        with pytest.raises(ValueError, match=text):
            _task(sim, fly, n_act, n_q, **over)
    unchanged()
    assert lib.nmf_task_update(None, None) != 0 and b"null task" in lib.nmf_last_error()
    assert lib.nmf_task_reset(None, None, None) != 0 and b"null task" in lib.nmf_last_error()
    h = live._handle()
    assert not lib.nmf_task_field_ptr(h, 19, None) and b"no such field" in lib.nmf_last_error()
    assert not lib.nmf_task_field_ptr(h, -1, None) and b"no such field" in lib.nmf_last_error()
    for bad, text in ((np.ones((n, 3)), "course"), (np.ones(3), "course")):
        with pytest.raises(ValueError, match=text):
            live.set_course(bad)
    with pytest.raises(ValueError, match="goal"):
        live.set_goal(np.ones((n + 1, 2)))
    with pytest.raises(ValueError, match="reset mask"):
        live.reset(np.ones(n + 1, dtype=bool))
    unchanged()

    # a following valid creation works
    h2 = create()
    assert h2
    width = ctypes.c_int32(0)
    assert lib.nmf_task_field_ptr(h2, 1, ctypes.byref(width)) and width.value == 18 + n_q
    assert lib.nmf_task_field_ptr(h2, 5, ctypes.byref(width)) and width.value == 2
    assert lib.nmf_task_field_ptr(h2, 9, ctypes.byref(width)) and width.value == 1
    assert lib.nmf_task_update(h2, sim._stream()) == 0
    lib.nmf_task_destroy(h2)
    with _task(sim, fly, n_act, n_q) as a:                                         # set_course normalises a shared row
        a.set_course((3.0, 4.0))
        torch.cuda.synchronize()
        assert np.allclose(a.course.cpu().numpy(), [[0.6, 0.8]] * n, atol=1e-6)
        assert isinstance(a.stats(), dict) and a.stats()["episodes"] == 0
    unchanged()
    stats = live.stats()
    assert stats["episodes"] == int(before["episodes"].sum()) and set(stats["reasons"]) == {*spec.REASONS, "time_limit"}
    live.close()
    for call in (live.update, live.reset, live.stats):
        with pytest.raises(RuntimeError, match="closed"):
            call()
    assert live.obs is None and live.done is None and live.course is None
    with pytest.raises(ValueError, match="for_fly"):
        class Several:
            for_fly = None
        WalkingTask(Several(), fly.name)


def test_real_physics_once(torch_mod):
    """16 worlds walk under ``TurningCPG`` for 60 ticks of 20 steps on flat ground with the shipped defaults (a 40-tick time limit
    apart, so that episodes end).  The specification, fed the inputs recorded before each update, agrees bit for bit, and no world
    shows NONFINITE; the reason histogram and the mean reward are printed, nothing more is asserted about them."""
    torch = torch_mod
    from flygym_amd.controllers import TurningCPG
    from flygym_amd.tasks import TaskEnv, WalkingTask

    n, ticks = 16, 60
    sim, fly = _batch(n, copy=3)
    sim.reset()
    sim.warmup()
    with TurningCPG(sim, fly.name, table_steps=32) as cpg, WalkingTask(sim, fly.name, max_ticks=40) as task:
        io = _Inputs(torch, sim, task)
        st = spec.State(n, spec.Params.from_struct(task._params), task.n_q)
        rewards = []
        for k in range(ticks):
            cpg.step(20)
            recorded = io.read()
            task.update()
            got = _numpy(torch, [_clone(task)])
            sim.reset_worlds(task.done)
            cpg.reset(task.done)
            st.update(*recorded)
            _assert_same(got, _stacked([st.snapshot()]), ("tick", k))
            assert not (st.reason & spec.NONFINITE).any()
            rewards.append(st.reward.mean())
        stats = task.stats()
        assert stats["episodes"] == int(st.episodes.sum()) >= n
        print(f"real physics, {n} worlds x {ticks} ticks with the defaults: mean reward per tick {np.mean(rewards):.4f}, {stats}")
        env = TaskEnv(sim, cpg, task)
        assert env.reset() is task.obs
