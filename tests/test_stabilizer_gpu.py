"""The head stabilizer on the GPU (``flygym_amd/csrc/nmf_stabilizer.hip``, ``flygym_amd.controllers.HeadStabilizer``) against its
numpy specification ``tests/stabilizer_spec.py``.

The inputs are synthetic except in the captured-tick test: after ``sim.reset()`` the tests write chosen joint angles and sensor
rows into the zero-copy views ``qpos`` and ``sensordata`` of the batch; nothing steps in between, so the inputs are exactly known.
The comparison rule: ``out`` equals the specification's bytes after every update.  ``tests/test_stabilizer_cpu.py`` asserts what
these inputs cover (every hidden unit active and clipped, every flag both ways, every output clamped at both ends and not)."""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest

import stabilizer_spec as spec

pytestmark = pytest.mark.gpu

KEYS = ("qpos", "qvel", "ctrl", "seg_xpos", "seg_xquat", "sensordata", "time")


@pytest.fixture
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch


@functools.lru_cache(maxsize=None)
def _batch(n):
    from flygym_amd import HIPSimulation, make_model

    fly, world, _ = make_model()
    sim = HIPSimulation(world, n_worlds=n, device=0)
    sim.set_leg_adhesion_states(fly.name, np.ones((n, 6), dtype=np.float32))
    sim.reset()
    return sim, fly


def _neck_fly():
    """An ALL_BIOLOGICAL fly on flat ground with the benchmark model's leg actuators and adhesion, and position actuators on the
    neck's roll and pitch — added FIRST, so that the leg columns of the CPG are not the leading position actuators."""
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


@functools.lru_cache(maxsize=None)
def _neck_batch(n, copy=0):
    from flygym_amd import HIPSimulation

    fly, world = _neck_fly()
    sim = HIPSimulation(world, n_worlds=n, device=0)
    sim.set_leg_adhesion_states(fly.name, np.ones((n, 6), dtype=np.float32))
    sim.reset()
    return sim, fly


def _stabilizer(sim, fly, name, **over):
    """The stabilizer of a parity case of the specification module on ``make_model()``'s fly, filling ``out`` only."""
    from flygym_amd.controllers import HeadStabilizer

    net = spec.network(name)
    names = [d.name for d in fly.get_jointdofs_order()]
    kw = dict(input_dofs=None if name == "default" else [names[i] for i in net.dof], input_mean=net.mean, input_std=net.std,
              contact_force_thr=spec.THR if net.contacts else None, limits=spec.bounds(name), drive_actuators=False)
    stab = HeadStabilizer(sim, fly.name, list(net.layers), **{**kw, **over})
    assert stab._dof.tolist() == net.dof.tolist() and stab._inv_std.tobytes() == net.inv_std.tobytes() and (stab.n_in, stab.n_out) == (net.n_in, net.n_out)
    assert not net.contacts or stab.thr2.tobytes() == net.thr2.tobytes()
    return stab


def _write_inputs(sim, q, sd):
    sim.field("qpos")[:, 7:].copy_(q)
    sim.field("sensordata").copy_(sd)


@functools.lru_cache(maxsize=None)
def _gpu_run(name, n):
    """The updates of an n-world batch on the device from the specification module's inputs: ``out`` after every update, as numpy
    (T, n, n_out).  The 65-world runs write into a caller's tensor, the others into the handle's own array."""
    import torch

    sim, fly = _batch(n)
    sim.reset()
    q, sd = (torch.as_tensor(np.array(a), device=sim.device) for a in spec.input_run(n))
    assert tuple(sim.field("qpos").shape) == (n, 7 + spec.N_DOF) and tuple(sim.field("sensordata").shape) == (n, 96)
    with _stabilizer(sim, fly, name) as stab:
        own = n != 65
        out = None if own else torch.full((n, stab.n_out), -7.0, dtype=torch.float32, device=sim.device)
        assert tuple(stab.output.shape) == (n, stab.n_out) and not bool(stab.output.any())
        clones = []
        for k in range(spec.UPDATES):
            _write_inputs(sim, q[k], sd[k])
            got = stab.update(out=out)
            assert got is (stab.output if own else out)
            clones.append(got.clone())
        torch.cuda.synchronize()
        if not own:                                                                # the handle's own array was never written
            assert not bool(stab.output.any())
        res = torch.stack(clones).cpu().numpy()
    res.setflags(write=False)
    return res


def _assert_same(got, want, where):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (where, got.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        first = [tuple(i) for i in bad[:4]]
        raise AssertionError((where, f"{len(bad)} of {got.size} values differ; first (update, world, output)", first,
                              [(float(got[i]), float(want[i])) for i in first]))


@pytest.mark.parametrize("n", spec.WORLDS)
@pytest.mark.parametrize("name", spec.PARITY + ("widest",))
def test_parity_with_the_specification(torch_mod, name, n):
    """1, 65 and 257 worlds (one lane past a wave, one past four waves) of the default 48 -> 32 -> 32 -> 2 network, the smallest
    (one joint angle, no contacts, one hidden unit, one output), a ragged one at the limits (66 + 6 inputs, hidden 33, 64, 7,
    8 outputs) and the widest (250 + 6 inputs: the largest LDS image), four updates each: ``out`` equals the specification's bytes
    after every update."""
    want, _ = spec.reference_run(name, n)
    got = _gpu_run(name, n)
    _assert_same(got, np.asarray(want), (name, n))
    print(f"stabilizer parity, {name}, {n} worlds x {spec.UPDATES} updates: {got.size} outputs bit for bit")


@pytest.mark.parametrize("name", spec.PARITY)
def test_a_world_does_not_depend_on_its_batch(torch_mod, name):
    """The last world of the 1-, 65- and 257-world runs is given the same inputs: its outputs are byte-identical."""
    runs = [_gpu_run(name, n) for n in spec.WORLDS]
    for other in runs[1:]:
        assert runs[0][:, 0].tobytes() == other[:, -1].tobytes()
    assert len(np.unique(runs[-1])) > 3                                            # (not one constant)


def _neck_network(fly, bias=(0.3, -0.2)):
    """The default network's weights with non-zero output biases, for the fly's own default inputs."""
    net = spec.network("default")
    (W0, b0), (W1, b1), (W2, _) = net.layers
    return [(W0, b0), (W1, b1), (0.05 * W2, np.array(bias, dtype=np.float32))]


def test_driving_ctrl(torch_mod):
    """A fly whose neck is actuated, 11 worlds, synthetic inputs: the ctrl columns of the neck's two actuators equal ``out`` as
    bytes and ``out`` equals the specification's; every other ctrl column, qpos, qvel and sensordata are untouched; with ``out=``
    given the handle's own array keeps its old contents."""
    torch = torch_mod
    from flygym_amd.controllers import NECK_DOFS, HeadStabilizer

    n = 11
    sim, fly = _neck_batch(n)
    sim.reset()
    dev = sim.device
    rng = np.random.default_rng(12)
    nj = sim.model.nq - 7
    q = rng.normal(0, 1, (2, n, nj)).astype(np.float32)
    _, sd = spec.input_run(n, 2)
    layers = _neck_network(fly)
    with HeadStabilizer(sim, fly.name, layers, limits=((-0.25, -0.5), (0.35, 0.1))) as stab:
        acts = [a["jointdof"].name for a in fly.actuators if a["kind"] == "position"]
        assert stab._act.tolist() == [acts.index(d) for d in NECK_DOFS] == [0, 43] and stab.n_in == 48 and len(set(stab._dof.tolist())) == 42
        net = dataclasses.replace(spec.network("default"), dof=stab._dof, mean=np.zeros(42, np.float32), std=np.ones(42, np.float32), layers=tuple(layers))
        ctrl = sim.field("ctrl")
        ctrl.copy_(torch.as_tensor(rng.normal(0, 1, tuple(ctrl.shape)).astype(np.float32), device=dev))
        others = [c for c in range(ctrl.shape[1]) if c not in stab._act.tolist()]
        for k, out in enumerate((None, torch.full((n, 2), -7.0, dtype=torch.float32, device=dev))):
            _write_inputs(sim, torch.as_tensor(q[k], device=dev), torch.as_tensor(np.array(sd[k]), device=dev))
            before = {key: sim.field(key).clone() for key in KEYS}
            own = stab.output.clone()
            got = stab.update(out=out)
            torch.cuda.synchronize()
            want, _ = spec.forward(net, q[k], sd[k], stab.lo, stab.hi)
            _assert_same(got.cpu().numpy(), want, ("driving ctrl", k))
            assert ctrl[:, stab._act.tolist()].cpu().numpy().tobytes() == want.tobytes()
            assert torch.equal(ctrl[:, others], before["ctrl"][:, others])
            for key in KEYS:
                if key != "ctrl":
                    assert torch.equal(sim.field(key), before[key]), key
            if out is not None:
                assert torch.equal(stab.output, own) and bool(own.any())
        assert (want >= stab.lo).all() and (want <= stab.hi).all()


def test_one_control_tick_is_one_captured_graph(torch_mod):
    """An ALL_BIOLOGICAL fly with neck roll / pitch position actuators under a ``TurningCPG`` (whose columns are the leg dofs among
    the position actuators).  Two settled 11-world batches: eight eager ticks of ``stab.update(); cpg.step(20)`` on one against one
    capture replayed eight times on the other: all batch fields and ``output`` are identical, and the specification, fed the qpos
    and sensordata recorded before each eager update, agrees bit for bit.  The network has non-zero output biases: against a third
    batch without a stabilizer the neck's joint angles differ at the end."""
    torch = torch_mod
    from flygym_amd.controllers import NECK_DOFS, HeadStabilizer, TurningCPG

    n, ticks, steps = 11, 8, 20
    sides = []
    for copy in (1, 2, 3):
        sim, fly = _neck_batch(n, copy=copy)
        sim.reset()
        sim.warmup()
        cpg = TurningCPG(sim, fly.name, table_steps=32)
        cpg.set_drive(np.tile(np.array([[1.0, 0.6]], dtype=np.float32), (n, 1)))
        stab = HeadStabilizer(sim, fly.name, _neck_network(fly)) if copy != 3 else None
        if stab is not None:
            stab.update()                                                          # one whole tick before the capture
        cpg.step(steps)
        sides.append((sim, cpg, stab))
    torch.cuda.synchronize()
    (s0, c0, h0), (s1, c1, h1), (s2, c2, _) = sides
    acts = [a["jointdof"].name for a in fly.actuators if a["kind"] == "position"]
    assert len(acts) == 44 and c0.act_ids.cpu().tolist() == [i for i, d in enumerate(acts) if d not in NECK_DOFS] and c0.n_act == 42
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        h1.update()
        c1.step(steps)
    net = dataclasses.replace(spec.network("default"), dof=h0._dof, mean=np.zeros(42, np.float32), std=np.ones(42, np.float32), layers=tuple(_neck_network(fly)))
    flags = np.zeros(6, dtype=bool)
    for k in range(ticks):
        torch.cuda.synchronize()
        q, sd = s0.field("qpos")[:, 7:].cpu().numpy().copy(), s0.field("sensordata").cpu().numpy().copy()
        h0.update()
        eager = h0.output.clone()
        c0.step(steps)
        g.replay()
        c2.step(steps)
        torch.cuda.synchronize()
        want, trace = spec.forward(net, q, sd, h0.lo, h0.hi)
        flags |= trace["flags"].any(axis=0)
        _assert_same(eager.cpu().numpy(), want, ("tick", k))
        assert torch.equal(h0.output, h1.output), k
        for key in KEYS:
            assert torch.equal(s0.field(key), s1.field(key)), (k, key)
    names = [d.name for d in fly.get_jointdofs_order()]
    cols = [7 + names.index(d) for d in NECK_DOFS]
    with_neck, without = s0.field("qpos")[:, cols].cpu().numpy(), s2.field("qpos")[:, cols].cpu().numpy()
    print(f"stabilizer in the captured tick, {n} worlds x {ticks} ticks: legs that touched above threshold {flags.tolist()}, "
          f"outputs now {want[0].tolist()}, neck angles {with_neck[0].tolist()} against {without[0].tolist()} without")
    assert np.isfinite(with_neck).all() and (with_neck != without).all()
    assert torch.equal(s0.field("ctrl")[:, h0._act.tolist()], h0.output)
    for _, cpg, stab in sides:
        if stab is not None:
            stab.close()
        cpg.close()


def test_refusals_leave_everything_untouched(torch_mod):
    """Every refused creation returns its message at the C ABI and leaks nothing (a following valid creation works); a misaligned
    ``out``, null handles and a closed handle are refused; so are wrong shapes, dtypes and devices in Python, and a missing neck
    actuator (a ``ValueError`` that names ``add_actuators``).  A live stabilizer's output and the batch read the same afterwards."""
    torch = torch_mod
    from flygym_amd import _native
    from flygym_amd.controllers import HeadStabilizer, _StabilizerParams

    lib = _native.lib()
    n = 11
    sim, fly = _batch(n)
    sim.reset()
    dev = sim.device
    q, sd = (torch.as_tensor(np.array(a), device=dev) for a in spec.input_run(n))
    _write_inputs(sim, q[0], sd[0])
    live = _stabilizer(sim, fly, "default")
    live.update()
    torch.cuda.synchronize()
    before = {key: sim.field(key).clone() for key in KEYS}
    own = live.output.clone()
    assert bool(own.any())

    def unchanged():
        torch.cuda.synchronize()
        assert torch.equal(live.output, own) and all(torch.equal(sim.field(key), before[key]) for key in KEYS)

    net = spec.network("default")
    nu = sim.model.nu

    def create(act=None, n_arrays=None, **over):
        """nmf_stabilizer_create with the live stabilizer's arguments, params fields and array entries overridden."""
        p = _StabilizerParams.from_buffer_copy(live._params)
        arrays = dict(dof=live._dof.copy(), mean=live._mean.copy(), inv_std=live._inv_std.copy(), weights=live._weights.copy())
        if n_arrays:                                                               # room for a larger n_q
            arrays = {k: np.resize(v, max(n_arrays, v.size) if k != "weights" else 40000) for k, v in arrays.items()}
            arrays["weights"][live._weights.size:] = 0
        for key, value in over.items():
            if key in arrays:
                arrays[key][value[0]] = value[1]
            elif isinstance(value, tuple):
                getattr(p, key)[value[0]] = value[1]
            else:
                setattr(p, key, value)
        a = None if act is None else np.array(act, dtype=np.int32)
        return lib.nmf_stabilizer_create(sim._batch_h, ctypes.byref(p), arrays["dof"].ctypes.data, arrays["mean"].ctypes.data,
                                         arrays["inv_std"].ctypes.data, arrays["weights"].ctypes.data, None if a is None else a.ctypes.data)

    nan, inf = float("nan"), float("inf")
    last_bias = live._weights.size - 1
    refusals = [(dict(n_hidden=0), b"n_hidden"), (dict(n_hidden=4), b"n_hidden"), (dict(hidden=(0, 0)), b"hidden[0]"), (dict(hidden=(1, 65)), b"hidden[1]"),
                (dict(n_q=0), b"n_q"), (dict(n_q=-3), b"n_q"), (dict(n_q=251, n_arrays=256), b"n_in"), (dict(n_q=257, n_arrays=260), b"n_in"),
                (dict(n_out=0), b"n_out"), (dict(n_out=9), b"n_out"),
                (dict(dof=(5, -1)), b"dof[5]"), (dict(dof=(41, spec.N_DOF)), b"dof[41]"),
                (dict(act=[0, nu]), b"act[1]"), (dict(act=[-1, 0]), b"act[0]"),
                (dict(lo=(1, 0.5), hi=(1, 0.25)), b"lo[1] > hi[1]"),
                (dict(weights=(7, nan)), b"layer 0 is not finite"), (dict(weights=(last_bias, inf)), b"layer 2 is not finite"),
                (dict(weights=(48 * 32 + 3, -inf)), b"layer 0 is not finite"),
                (dict(mean=(3, nan)), b"not finite at input 3"), (dict(inv_std=(41, inf)), b"not finite at input 41"),
                (dict(thr2=(4, nan)), b"thr2 is not finite at leg 4"), (dict(lo=(0, -inf)), b"bound is not finite"), (dict(hi=(1, nan)), b"bound is not finite")]
    for over, text in refusals:
        assert not create(**over) and text in lib.nmf_last_error(), (over, lib.nmf_last_error())
        unchanged()
    good = (live._dof.ctypes.data, live._mean.ctypes.data, live._inv_std.ctypes.data, live._weights.ctypes.data, None)
    assert not lib.nmf_stabilizer_create(None, ctypes.byref(live._params), *good) and b"null" in lib.nmf_last_error()
    assert not lib.nmf_stabilizer_create(sim._batch_h, None, *good) and b"null" in lib.nmf_last_error()
    for missing in range(4):
        args = [*good]
        args[missing] = None
        assert not lib.nmf_stabilizer_create(sim._batch_h, ctypes.byref(live._params), *args) and b"null" in lib.nmf_last_error()
    unchanged()

    # the Python class raises NativeError with the library's message, or ValueError before it gets there
    with pytest.raises(_native.NativeError, match=r"lo\[0\] > hi\[0\]"):
        _stabilizer(sim, fly, "default", limits=(0.5, -0.5))
    with pytest.raises(_native.NativeError, match=r"hidden\[0\] must be in 1..64"):
        HeadStabilizer(sim, fly.name, [(np.zeros((65, 48), np.float32), np.zeros(65, np.float32)), (np.zeros((2, 65), np.float32), np.zeros(2, np.float32))],
                       drive_actuators=False)
    with pytest.raises(_native.NativeError, match="not finite"):
        _stabilizer(sim, fly, "default", input_mean=np.full(42, nan, np.float32))
    with pytest.raises(ValueError, match="layer 1"):
        HeadStabilizer(sim, fly.name, [net.layers[0], net.layers[0]], drive_actuators=False)
    with pytest.raises(ValueError, match="layers"):
        HeadStabilizer(sim, fly.name, [net.layers[0]], drive_actuators=False)
    with pytest.raises(ValueError, match="input_std"):
        _stabilizer(sim, fly, "default", input_std=np.zeros(42, np.float32))
    with pytest.raises(ValueError, match="no joint dof"):
        _stabilizer(sim, fly, "default", input_dofs=["c_thorax-c_head-roll"] * 42)
    with pytest.raises(ValueError, match="contact_force_thr"):
        _stabilizer(sim, fly, "default", contact_force_thr=(1.0, 2.0))
    with pytest.raises(ValueError, match="add_actuators"):                        # a LEGS_ONLY fly has no neck to drive
        HeadStabilizer(sim, fly.name, list(net.layers))
    with pytest.raises(ValueError, match="2 outputs for 1 output dofs"):
        HeadStabilizer(sim, fly.name, list(net.layers), output_dofs=["c_thorax-c_head-roll"])
    with pytest.raises(ValueError, match="no fly named"):
        HeadStabilizer(sim, "nobody", list(net.layers), drive_actuators=False)
    with pytest.raises(ValueError, match="for_fly"):
        class Several:
            for_fly = None
        HeadStabilizer(Several(), fly.name, list(net.layers), drive_actuators=False)
    unchanged()

    # refused updates at the C ABI, null handles
    h, stream = live._handle(), sim._stream()
    out = torch.zeros((n, 2), dtype=torch.float32, device=dev)
    for offset in (4, 8, 12):
        assert lib.nmf_stabilizer_update(h, out.data_ptr() + offset, stream) != 0 and b"16-byte aligned" in lib.nmf_last_error()
    assert lib.nmf_stabilizer_update(None, out.data_ptr(), stream) != 0 and b"null stabilizer" in lib.nmf_last_error()
    assert not lib.nmf_stabilizer_field_ptr(None, 0, None) and b"null stabilizer" in lib.nmf_last_error()
    assert not lib.nmf_stabilizer_field_ptr(h, 1, None) and b"no such field" in lib.nmf_last_error()
    assert not lib.nmf_stabilizer_field_ptr(h, -1, None) and b"no such field" in lib.nmf_last_error()
    lib.nmf_stabilizer_destroy(None)
    unchanged()
    assert not bool(out.any())

    # wrong shapes, dtypes and devices, in Python
    bad = [torch.zeros((n, 3), device=dev), torch.zeros((n + 1, 2), device=dev), torch.zeros((n, 2), dtype=torch.float64, device=dev),
           torch.zeros((n, 2)), torch.zeros((n, 4), device=dev)[:, :2], torch.zeros((2, n), device=dev).T, np.zeros((n, 2), np.float32)]
    for x in bad:
        with pytest.raises(ValueError, match="out must be"):
            live.update(out=x)
    unchanged()

    # a following valid creation works
    h2 = create()
    assert h2
    width = ctypes.c_int32(0)
    assert lib.nmf_stabilizer_field_ptr(h2, 0, ctypes.byref(width)) and width.value == 2
    assert lib.nmf_stabilizer_update(h2, out.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, own)
    lib.nmf_stabilizer_destroy(h2)
    unchanged()
    live.close()
    with pytest.raises(RuntimeError, match="closed"):
        live.update()
    assert live.output is None
