"""Rule-based walking on the GPU (``flygym_amd/csrc/nmf_rules.hip``, ``flygym_amd.controllers.RuleBasedController``) against its
numpy specification ``tests/rules_spec.py``.

The comparison rule: after every launch every view and rows ``0 .. n_steps - 1`` of the table equal the specification's bit for bit
(floats compared as bytes).  ``tests/test_rules_cpu.py`` asserts that the drive schedule used here exercises what the kernel can get
wrong."""
import ctypes
import functools

import numpy as np
import pytest

import rules_spec as spec

pytestmark = pytest.mark.gpu

FIELDS = spec.FIELDS
P = spec.PARITY


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


def _controller(sim, fly, **over):
    """A controller with the parity settings of the specification module (``spec.PARITY``)."""
    from flygym_amd.controllers import RuleBasedController

    return RuleBasedController(sim, fly.name, **{**P, **over})


def _clone(ctl):
    return {name: getattr(ctl, name).clone() for name in FIELDS}


def _numpy(torch, clones):
    """A list of per-launch dicts of device tensors -> a list of dicts of numpy arrays."""
    torch.cuda.synchronize()
    got = [{name: c[name].cpu().numpy() for name in c} for c in clones]
    for g in got:
        g["ticks"] = g["ticks"].view(np.uint32)                                    # (the view shows the uint32 counter as int32)
    return got


def _assert_same(got, want, where):
    for name in want:
        g, w = got[name], want[name]
        assert g.dtype == w.dtype and g.shape == w.shape, (where, name, g.dtype, w.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            gb, wb = (np.ascontiguousarray(a).view(np.uint8).reshape(*a.shape, -1) for a in (g, w))
            first = [tuple(i) for i in np.argwhere((gb != wb).any(axis=-1))[:3]]
            raise AssertionError((where, name, "first differences at (world, ...)", first, [(g[i], w[i]) for i in first]))


def _assert_tables_match(ctl, adhesion):
    """The controller built the tables the CPU tests studied."""
    want, got = spec.tables(P["n_phase_bins"], P["period_steps"], adhesion), spec.Tables.of(ctl)
    for name in ("cycle", "leg_of_col", "start_bin", "swing_steps", "weights"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), name
    assert (got.period_steps, got.margin, got.max_amplitude, got.adhesion) == (want.period_steps, want.margin, want.max_amplitude, want.adhesion)


@functools.lru_cache(maxsize=None)
def _gpu_run(n, adhesion, first_world=spec.FIRST, worlds=None):
    """``spec.LAUNCHES`` on an n-world batch under ``spec.input_run``'s drives (``worlds``: as ``spec.reference_run``); per launch
    the rows written and every view, as numpy."""
    import torch

    sim, fly = _batch(n)
    drives = spec.input_run(n) if worlds is None else spec.input_run(worlds[2])[:, worlds[0]:worlds[1]]
    clones = []
    with _controller(sim, fly, adhesion=adhesion, first_world=first_world) as ctl:
        _assert_tables_match(ctl, adhesion)
        assert tuple(ctl.table.shape) == (n, 64, 42 + (6 if adhesion else 0)) and tuple(ctl.ticks.shape) == (n,)
        for launch, n_steps in enumerate(spec.LAUNCHES):
            ctl.set_drive(np.array(drives[launch]))
            table = ctl.advance(n_steps)
            clones.append(dict(_clone(ctl), rows=table[:, :n_steps].clone()))
        got = _numpy(torch, clones)
    for g in got:
        for a in g.values():
            a.setflags(write=False)
    return got


@pytest.mark.parametrize("adhesion", [None, spec.ADHESION])
@pytest.mark.parametrize("n", spec.CASES)
def test_parity_with_the_specification(torch_mod, n, adhesion):
    """1, 10, 11 and 23 worlds (one world, a full workgroup, one world into the second, a partial third), ten launches of 1, 31, 32,
    33, 64 steps twice over (the 32-step pass boundary and table_steps; 322 steps, 13 periods of 24) with a new drive before each:
    worlds that stop for 65 steps and start again, worlds with one side at 0, amplitudes above max_amplitude.  16 bins over a period
    of 24 steps; with and without adhesion columns.  Every view and every row written equal the specification's bytes after every
    launch."""
    want, cover, _ = spec.reference_run(n, adhesion)
    got = _gpu_run(n, adhesion)
    for launch, ((rows, snap), g) in enumerate(zip(want, got)):
        _assert_same(g, dict(snap, rows=rows), (n, adhesion, "launch", launch))
    assert (got[-1]["ticks"] == sum(spec.LAUNCHES)).all() and cover["completions"] >= 20
    print(f"rules parity, {n} worlds x {sum(spec.LAUNCHES)} steps, adhesion {adhesion}: all views and rows bit for bit; {cover}")


def test_the_default_shape_once(torch_mod):
    """256 bins, the default period (833 steps at 0.1 ms) and weights, adhesion columns, 11 worlds, one 64-step launch."""
    torch = torch_mod
    from flygym_amd.controllers import RuleBasedController

    sim, fly = _batch(11)
    with RuleBasedController(sim, fly.name, adhesion=spec.ADHESION, seed=3) as ctl:
        assert ctl.period_steps == round(1.0 / (12.0 * sim.timestep)) == 833 and ctl.n_bins == 256 and ctl.table_steps == 64
        st = spec.State(11, spec.Tables.of(ctl), seed=3)
        rows = st.advance(64)
        table = ctl.advance(64)
        got = _numpy(torch, [dict(_clone(ctl), rows=table.clone())])[0]
    _assert_same(got, dict(st.snapshot(), rows=rows), "default shape")
    assert (got["counter"].max(axis=1) == 64).all() and (got["ticks"] == 64).all()


def test_masked_reset(torch_mod):
    """23 worlds; after three launches the odd ones are reset: they equal a fresh controller's, the others are untouched, as bytes;
    two more launches follow a specification reset the same way."""
    torch = torch_mod
    n = 23
    sim, fly = _batch(n)
    drives = spec.input_run(n)
    mask = np.arange(n) % 2 == 1
    st = spec.State(n, spec.tables(P["n_phase_bins"], P["period_steps"]), seed=spec.SEED, first_world=spec.FIRST)
    with _controller(sim, fly) as ctl, _controller(sim, fly) as fresh:
        def run(launches):
            for launch in launches:
                ctl.set_drive(np.array(drives[launch])); st.drive[:] = drives[launch]
                table = ctl.advance(spec.LAUNCHES[launch])
                rows = st.advance(spec.LAUNCHES[launch])
                got = _numpy(torch, [dict(_clone(ctl), rows=table[:, :spec.LAUNCHES[launch]].clone())])[0]
                _assert_same(got, dict(st.snapshot(), rows=rows), ("masked reset, launch", launch))

        run((0, 1, 2))
        before = _numpy(torch, [_clone(ctl)])[0]
        assert before["counter"][mask].any() and before["stepping"][mask].any() and (before["ticks"] == 64).all()
        ctl.reset(torch.as_tensor(mask))
        st.reset(mask)
        after, new = _numpy(torch, [_clone(ctl), _clone(fresh)])
        for name in FIELDS:
            assert after[name][mask].tobytes() == new[name][mask].tobytes(), name
            assert after[name][~mask].tobytes() == before[name][~mask].tobytes(), name
        assert not after["counter"][mask].any() and not after["ticks"][mask].any() and (after["amplitude"][mask] == 1).all()
        assert (after["drive"][mask] == 1).all() and not after["scores"][mask].any() and not after["stepping"][mask].any()
        run((3, 4))
        # a reset of every world, from a numpy mask and from none
        ctl.reset(np.ones(n, dtype=bool)); fresh.reset()
        both = _numpy(torch, [_clone(ctl), _clone(fresh)])
        assert all(both[0][name].tobytes() == both[1][name].tobytes() for name in FIELDS) and not both[0]["ticks"].any()


def test_a_world_does_not_depend_on_its_shard(torch_mod):
    """Worlds 5..15 of the 23-world batch equal, in every view and row after every launch, an 11-world batch created with
    first_world moved by 5 and given their drives: other lanes, other workgroups."""
    whole = _gpu_run(23, None)
    shard = _gpu_run(11, None, first_world=spec.FIRST + 5, worlds=(5, 16, 23))
    for launch, (a, b) in enumerate(zip(whole, shard)):
        for name in (*FIELDS, "rows"):
            assert a[name][5:16].tobytes() == b[name].tobytes(), (launch, name)
    want, _, _ = spec.reference_run(11, None, spec.FIRST + 5, (5, 16, 23))
    for launch, ((rows, snap), g) in enumerate(zip(want, shard)):
        _assert_same(g, dict(snap, rows=rows), ("shard, launch", launch))
    # and it does depend on the global index: the same drives at another first_world decide otherwise
    other = _gpu_run(11, None, first_world=spec.FIRST + 6, worlds=(5, 16, 23))
    assert other[-1]["counter"].tobytes() != shard[-1]["counter"].tobytes()


def test_one_control_tick_is_one_captured_graph(torch_mod):
    """``torch.cuda.graph`` over ``ctl.step(20)`` on 16 settled worlds, replayed 5 times, equals the specification advanced 100
    steps, after every replay: the tick word moves and fresh draws are taken on every replay."""
    torch = torch_mod
    n = 16
    sim, fly = _batch(n, copy=1)
    sim.warmup()
    with _controller(sim, fly, adhesion=spec.ADHESION, table_steps=32) as ctl:
        ctl.step(20)                                                               # every kernel of the tick has run before the capture
        ctl.reset()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ctl.step(20)
        assert not bool(ctl.ticks.any()) and not bool(ctl.counter.any())            # (the capture itself ran nothing)
        st = spec.State(n, spec.Tables.of(ctl), seed=spec.SEED, first_world=spec.FIRST)
        for k in range(5):
            g.replay()
            rows = st.advance(20)
            got = _numpy(torch, [dict(_clone(ctl), rows=ctl.table[:, :20].clone())])[0]
            _assert_same(got, dict(st.snapshot(), rows=rows), ("replay", k))
            assert (got["ticks"] == 20 * (k + 1)).all()
        starts = len(st.starts)
        assert starts >= 3 * n and bool(torch.isfinite(sim.field("qpos")).all())
    print(f"rules in a captured tick, {n} worlds x 5 replays of 20 steps: {starts} steps started, all views and rows bit for bit")


def test_the_controller_drives_the_batch(torch_mod):
    """16 settled worlds, 10 ticks of ``step(20)`` with adhesion: ``ctrl`` at the controller's ``act_ids`` equals the last row
    written, the state is finite and the leg joint angles have moved.  (No bar on how well it walks.)"""
    torch = torch_mod
    from flygym_amd.controllers import RuleBasedController

    n = 16
    sim, fly = _batch(n, copy=2)
    sim.warmup()
    with RuleBasedController(sim, fly.name, adhesion=spec.ADHESION) as ctl:
        q0 = sim.get_joint_angles(fly.name).clone()
        for _ in range(10):
            ctl.step(20)
        torch.cuda.synchronize()
        ctrl = sim.field("ctrl")[:, ctl.act_ids.long()]
        assert torch.equal(ctrl, ctl.table[:, 19]) and int(ctl.ticks[0]) == 200
        assert all(bool(torch.isfinite(sim.field(key)).all()) for key in ("qpos", "qvel", "ctrl", "seg_xpos"))
        moved = float((sim.get_joint_angles(fly.name) - q0).abs().max())
        print(f"rules drive the batch: largest joint-angle change after 200 steps {moved:.3f} rad, legs stepping now "
              f"{ctl.stepping.sum(dim=1).tolist()}")
        assert moved > 0.05 and bool((ctl.stepping.sum(dim=1) >= 1).all())


def _neck_fly():
    """An ALL_BIOLOGICAL fly on flat ground with the benchmark model's leg actuators and adhesion, and position actuators on the
    neck's roll and pitch — the first added before the legs', so that the leg columns are not the leading position actuators."""
    import flygym_amd.compose as C
    from flygym_amd import anatomy as A
    from flygym_amd.controllers import NECK_DOFS
    from flygym_amd.utils.math import Rotation3D

    fly = C.Fly(name="t")
    fly.add_joints(A.Skeleton(axis_order=A.AxisOrder.YAW_PITCH_ROLL, joint_preset=A.JointPreset.ALL_BIOLOGICAL), neutral_pose=C.KinematicPosePreset.NEUTRAL)
    fly.add_actuators([A.JointDOF.from_name(NECK_DOFS[0])], C.ActuatorType.POSITION, kp=50.0)
    legs = A.Skeleton(axis_order=A.AxisOrder.YAW_PITCH_ROLL, joint_preset=A.JointPreset.LEGS_ONLY)
    fly.add_actuators(legs.get_actuated_dofs_from_preset("legs_active_only"), C.ActuatorType.POSITION, kp=50.0,
                      neutral_input=C.KinematicPosePreset.NEUTRAL)
    fly.add_actuators([A.JointDOF.from_name(NECK_DOFS[1])], C.ActuatorType.POSITION, kp=50.0)
    fly.add_leg_adhesion()
    world = C.FlatGroundWorld()
    world.add_fly(fly, (0, 0, 0.8), Rotation3D("quat", (1, 0, 0, 0)))
    return fly, world


def test_a_fly_with_neck_actuators(torch_mod):
    """Position actuators beyond the legs: the table has only the 42 leg columns (and the adhesion ones), ``act_ids`` name the legs'
    controls, and the neck's controls are not written."""
    torch = torch_mod
    from flygym_amd import HIPSimulation
    from flygym_amd.controllers import RuleBasedController, TurningCPG

    fly, world = _neck_fly()
    sim = HIPSimulation(world, n_worlds=3, device=0)
    sim.set_leg_adhesion_states(fly.name, np.ones((3, 6), dtype=np.float32))
    sim.reset()
    with RuleBasedController(sim, fly.name, adhesion=spec.ADHESION, **P) as ctl, TurningCPG(sim, fly.name, adhesion=spec.ADHESION) as cpg:
        assert ctl.n_act == 48 and tuple(ctl.table.shape) == (3, 64, 48) and ctl.n_given == 44 and len(ctl.actuated_dofs) == 42
        assert torch.equal(ctl.act_ids, cpg.act_ids) and ctl.act_ids.numel() == 48
        neck = [i for i in sim.replay_ids(fly.name).tolist() if i not in ctl.act_ids.tolist()]
        assert len(neck) == 2
        sim.field("ctrl")[:, neck] = 0.125
        ctl.step(5)
        torch.cuda.synchronize()
        assert torch.equal(sim.field("ctrl")[:, ctl.act_ids.long()], ctl.table[:, 4]) and bool((sim.field("ctrl")[:, neck] == 0.125).all())
        st = spec.State(3, spec.Tables.of(ctl), seed=spec.SEED, first_world=spec.FIRST)
        assert np.array_equal(st.advance(5), ctl.table[:, :5].cpu().numpy())


def test_validation(torch_mod):
    """The ``ValueError`` s of the class, the library's own refusals, and a closed controller."""
    torch = torch_mod
    from flygym_amd import _native
    from flygym_amd.controllers import RuleBasedController, _RulesParams

    n = 11
    sim, fly = _batch(n)
    make = lambda **kw: RuleBasedController(sim, fly.name, **kw)
    for bad, text in ((dict(table_steps=0), "table_steps"), (dict(n_phase_bins=1), "n_phase_bins"), (dict(period_steps=1), "period_steps"),
                      (dict(period_steps=2 ** 23, n_phase_bins=256), "period_steps"), (dict(frequency=0.0), "frequency"),
                      (dict(period_steps=2), "leaves no stance"), (dict(weights={"rule9": 1.0}), "weights takes the keys"),
                      (dict(rules_graph={"rule2": []}), "rules_graph takes the keys"), (dict(margin=-1.0), "margin"),
                      (dict(max_amplitude=float("nan")), "max_amplitude"), (dict(first_world=-1), "first_world"),
                      (dict(adhesion=(1.0,)), "adhesion"), (dict(adhesion=(20.0, 1.0, 1.5)), "swing in every bin|stance in every bin")):
        with pytest.raises(ValueError, match=text):
            make(**bad)
    with pytest.raises(ValueError, match="no fly named"):
        RuleBasedController(sim, "nosuchfly")
    with pytest.raises(ValueError, match="for_fly"):
        class Several:
            for_fly = None
        RuleBasedController(Several(), fly.name)
    ctl = make(**P)
    assert ctl.counter.dtype == torch.int32 and ctl.stepping.dtype == torch.uint8 and ctl.ticks.dtype == torch.int32
    assert tuple(ctl.counter.shape) == (n, 6) and tuple(ctl.drive.shape) == (n, 2) and tuple(ctl.scores.shape) == (n, 6)
    assert bool((ctl.drive == 1).all()) and bool((ctl.amplitude == 1).all())
    for bad in (0, 65, -3):
        with pytest.raises(ValueError, match="n_steps"):
            ctl.advance(bad)
        with pytest.raises(ValueError, match="n_steps"):
            ctl.step(bad)
    for bad in (np.ones((n, 3)), np.ones((n - 1, 2)), np.ones(2)):
        with pytest.raises(ValueError, match="Expected a drive of shape"):
            ctl.set_drive(bad)
    with pytest.raises(ValueError, match="reset mask"):
        ctl.reset(np.ones(n + 1, dtype=bool))
    # the library's own validation (a binding that skips the Python checks)
    lib = _native.lib()
    table = ctl.table.data_ptr()
    for args, text in (((0, table, 64), b"n_steps"), ((65, table, 64), b"n_steps"), ((1, None, 64), b"null table"),
                       ((1, table, 32), b"tables of 64 steps")):
        assert lib.nmf_rules_advance(ctl._h, args[0], args[1], args[2], None) != 0 and text in lib.nmf_last_error(), args
    cyc = np.ascontiguousarray(ctl.cycle, dtype=np.float32)
    legs = np.ascontiguousarray(ctl.leg_of_dof, dtype=np.int32)

    def create(legs=legs, start=ctl.start_bin, swing=ctl.swing_steps, weights=ctl.weights, **over):
        p = _RulesParams.from_buffer_copy(ctl._params)
        for key, value in over.items():
            setattr(p, key, value)
        return lib.nmf_rules_create(sim._batch_h, ctypes.byref(p), cyc.ctypes.data, legs.ctypes.data, start.ctypes.data, swing.ctypes.data,
                                    weights.ctypes.data)

    bad_legs = legs.copy(); bad_legs[7] = 6
    bad_start = ctl.start_bin.copy(); bad_start[2] = 16
    bad_swing = ctl.swing_steps.copy(); bad_swing[4] = 24
    no_swing = ctl.swing_steps.copy(); no_swing[0] = 0
    bad_weights = ctl.weights.copy(); bad_weights[1, 2, 3] = np.inf
    refusals = [(dict(legs=bad_legs), b"leg_of_col[7]"), (dict(start=bad_start), b"start_bin[2]"), (dict(swing=bad_swing), b"swing_steps[4]"),
                (dict(swing=no_swing), b"swing_steps[0]"), (dict(weights=bad_weights), b"weight is not finite"), (dict(n_bins=1), b"n_bins"),
                (dict(n_pos=0), b"n_pos"), (dict(period_steps=1), b"period_steps"), (dict(period_steps=2 ** 27), b"2^31"),
                (dict(table_steps=0), b"table_steps"), (dict(margin=-0.5), b"margin"), (dict(max_amplitude=float("inf")), b"not finite"),
                (dict(first_world=-1), b"first_world")]
    for over, text in refusals:
        assert not create(**over) and text in lib.nmf_last_error(), (over, lib.nmf_last_error())
    assert not lib.nmf_rules_field_ptr(ctl._h, 6, None) and b"no such field" in lib.nmf_last_error()
    h2 = create()                                          # a following valid creation works
    assert h2
    width = ctypes.c_int32(0)
    assert lib.nmf_rules_field_ptr(h2, 3, ctypes.byref(width)) and width.value == 2
    assert lib.nmf_rules_field_ptr(h2, 4, ctypes.byref(width)) and width.value == 1
    lib.nmf_rules_destroy(h2)
    torch.cuda.synchronize()
    assert bool((ctl.table == 0).all()) and not bool(ctl.ticks.any())               # none of the refused calls wrote a row
    with ctl:
        pass
    for call in (lambda: ctl.advance(1), lambda: ctl.set_drive(np.ones((n, 2))), ctl.reset):
        with pytest.raises(RuntimeError, match="closed"):
            call()
    assert ctl.counter is None and ctl.drive is None and ctl.scores is None
    ctl.close()                                            # closing twice is fine
