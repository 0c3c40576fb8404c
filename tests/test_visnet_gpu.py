"""The retinotopic visual network on the GPU (``flygym_amd/csrc/nmf_visnet.hip``, ``flygym_amd.sensors.RetinotopicNetwork``)
against its numpy specification ``tests/visnet_spec.py``.

Every comparison with the specification is bit for bit: every chain of the kernel is the specification's sequence of ``fmaf``, its
pooled sums are integers of terms rounded before they are added, its quotients correctly rounded divisions of exact operands and
the rest of its float32 rule is compiled without contraction or reassociation."""
import ctypes
import functools

import numpy as np
import pytest

import visnet_spec as spec

pytestmark = pytest.mark.gpu

f32 = np.float32
VIEWS = ("v", "sums", "pooled", "signal", "drive", "fresh")
# (case, substeps): the cases of visnet_spec.case, and the default network on the default retina with the class's own tables
CASES = [("smallest", 1), ("ring", 2), ("ragged", 1), ("ragged", 3), ("widest", 1), ("square", 1), ("pathway", 1)]


@pytest.fixture
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == f32 else x.astype(np.int32)


@functools.lru_cache(maxsize=None)
def _plain_batch(n):
    """n worlds of the benchmark fly, never stepped: something for a RetinotopicNetwork to belong to."""
    from flygym_amd import HIPSimulation, make_model

    fly, world, _ = make_model()
    return HIPSimulation(world, n_worlds=n, device=0), fly


@functools.lru_cache(maxsize=None)
def _walking_batch(n, copy=0):
    """n settled worlds with leg adhesion on (one per size and copy)."""
    from flygym_amd import HIPSimulation, make_model

    fly, world, _ = make_model()
    sim = HIPSimulation(world, n_worlds=n, device=0)
    sim.set_leg_adhesion_states(fly.name, np.ones((n, 6), dtype=np.float32))
    sim.warmup()
    return sim, fly


@functools.lru_cache(maxsize=None)
def _case(name, substeps):
    """``(network for the class, Flat for the specification, neighbours (2, T, n_omm), retina)``."""
    from flygym_amd import sensors

    if name == "pathway":
        retina = spec.retina("default")
        table, offsets = sensors.eye_tables(retina, 1)                     # (the class's own choice: the taps reach one ring)
        network = sensors.motion_pathway(offsets)
        _, types, edges, taps, tap_w = sensors.flatten_network(network, spec.DT, substeps)
        flat = spec.Flat(types, edges, taps, tap_w, np.array([network.tau[t] for t in network.types]), substeps)
        return network, flat, table, retina
    flat, table, which = spec.case(name, substeps)
    network = sensors.FlatNetwork(types=tuple(f"c{c}" for c in range(flat.n_types)), tau=flat.tau, bias=flat.types[:, 0], in_w=flat.types[:, 1:3],
                                  steer_w=flat.types[:, 4], edges=flat.edges, taps=flat.taps, tap_w=flat.tap_w)
    return network, flat, spec.both_eyes(table).astype(np.int32), spec.retina(which)


@functools.lru_cache(maxsize=None)
def _reference(name, substeps, reset_at=None):
    """The specification's run of the whole population, computed once: a batch of n worlds is its last n."""
    _, flat, table, retina = _case(name, substeps)
    mask = np.array([1, 0, 1], dtype=bool) if reset_at is not None else None
    return spec.run(flat, table, retina.num_ommatidia, spec.N_TOTAL, reset_at=reset_at, reset_mask=mask)


def _assert_equal_bits(label, net, drive, state, want, rows=slice(None)):
    ref = {"v": state["v"], "sums": want["sums"], "pooled": want["pooled"], "signal": want["signal"], "drive": want["drive"]}
    for name, value in ref.items():
        got = (drive if name == "drive" else getattr(net, name)).cpu().numpy()
        same = _bits(got) == _bits(value[rows])
        assert same.all(), f"{label}: {name} differs in {int((~same).sum())} of {same.size} values, first at {np.argwhere(~same)[0].tolist()}"
    assert np.array_equal(net.fresh.cpu().numpy() != 0, state["fresh"][rows]), f"{label}: fresh"


def _make(torch, name, substeps, n, **extra):
    from flygym_amd.sensors import RetinotopicNetwork

    sim, fly = _plain_batch(n)
    network, flat, table, retina = _case(name, substeps)
    net = RetinotopicNetwork(sim, fly.name, network, dt=spec.DT, retina=retina, neighbours=None if name == "pathway" else table,
                             substeps=substeps, **{**spec.PARAMS, **extra})
    frames = torch.as_tensor(np.array(spec.readings(retina.num_ommatidia)[:, spec.N_TOTAL - n:]), device=sim.device)
    base = torch.as_tensor(np.array(spec.bases()[spec.N_TOTAL - n:]), device=sim.device)
    return sim, net, frames, base


@pytest.mark.parametrize("n", spec.WORLDS)
@pytest.mark.parametrize("name,substeps", CASES)
def test_the_kernel_equals_the_specification_bit_for_bit(torch_mod, name, substeps, n):
    """Four consecutive updates with changing readings, the scalar base and a base tensor in turn; a batch of one world is the
    last world of the batch of three, so a world's bytes depend neither on its batch nor on its place in it."""
    torch = torch_mod
    sim, net, frames, base = _make(torch, name, substeps, n)
    rows = slice(spec.N_TOTAL - n, None)
    with net:
        _, flat, table, retina = _case(name, substeps)
        C, n_omm = flat.n_types, retina.num_ommatidia
        assert tuple(net.v.shape) == (n, 2, C, n_omm) and tuple(net.pooled.shape) == tuple(net.sums.shape) == (n, 2, C)
        assert net.sums.dtype == torch.int32 and tuple(net.signal.shape) == (n,) and tuple(net.drive.shape) == tuple(net.fresh.shape) == (n, 2)
        assert np.array_equal(net.neighbours, table) and len(net.type_names) == C
        assert bool((net.fresh == 1).all()) and bool((net.drive == 1).all()) and bool((net.v == 0).all())
        for k, (state, want) in enumerate(_reference(name, substeps)):
            drive = net.update(frames[k], base=base if k % 2 else None)
            assert drive is net.drive
            torch.cuda.synchronize()
            _assert_equal_bits(f"{name}, substeps {substeps}, {n} worlds, update {k}", net, drive, state, want, rows)


def test_a_masked_reset_restarts_its_worlds_and_no_others(torch_mod):
    """Worlds 0 and 2 are reset before the third update: their cells restart from the bias, world 1 continues bit for bit."""
    torch = torch_mod
    sim, net, frames, base = _make(torch, "ragged", 3, 3)
    mask = np.array([1, 0, 1], dtype=bool)
    with net:
        plain = _reference("ragged", 3)
        for k, (state, want) in enumerate(_reference("ragged", 3, reset_at=2)):
            if k == 2:
                net.reset(mask)
                torch.cuda.synchronize()
                assert np.array_equal(net.fresh.cpu().numpy() != 0, np.stack([mask, mask], axis=-1))
            drive = net.update(frames[k], base=base if k % 2 else None)
            torch.cuda.synchronize()
            _assert_equal_bits(f"update {k}", net, drive, state, want)
            if k >= 2:
                assert np.array_equal(state["v"][1], plain[k][0]["v"][1]) and not np.array_equal(state["v"][0], plain[k][0]["v"][0])
        net.reset()
        torch.cuda.synchronize()
        assert bool((net.fresh == 1).all())


def test_a_base_tensor_stands_for_the_scalar_and_out_spares_the_own_drive(torch_mod):
    torch = torch_mod
    sim, net, frames, _ = _make(torch, "ring", 2, 3)
    _, twin, _, _ = _make(torch, "ring", 2, 3)
    with net, twin:
        big = torch.full((5, 2), -3.0, dtype=torch.float32, device=sim.device)
        for k in range(2):
            a = net.update(frames[k])
            b = twin.update(frames[k], base=torch.full((3, 2), spec.PARAMS["base"], dtype=torch.float32, device=sim.device), out=big[1:4])
            assert a is net.drive and b.data_ptr() == big[1:4].data_ptr()
            torch.cuda.synchronize()
            assert torch.equal(a, b) and torch.equal(net.v, twin.v) and torch.equal(net.signal, twin.signal)
            assert bool((twin.drive == 1).all()) and bool((big[0] == -3).all()) and bool((big[4] == -3).all())
        assert not bool((a == spec.PARAMS["base"]).all())                         # (the drive did move)


def test_one_control_tick_is_one_captured_graph(torch_mod):
    """Eye renderer + ``update(omm, out=cpg.drive)`` + ``cpg.step(20)`` captured once and replayed eight times on one batch of five
    worlds, against eight eager ticks on a twin batch: every field of the batch, the controller's state and every view of the
    network are identical."""
    torch = torch_mod
    from flygym_amd.controllers import TurningCPG
    from flygym_amd.sensors import RetinotopicNetwork, motion_pathway
    from flygym_amd.vision import EyeRenderer, Scene

    n = 5
    keys = ("qpos", "qvel", "ctrl", "qacc_warmstart", "seg_xpos", "seg_xquat", "site_xpos", "actuator_force", "sensordata", "time",
            "stats", "qacc", "stats_sum", "contact_geom", "act")
    runs = []
    for copy in (1, 2):
        sim, fly = _walking_batch(n, copy)
        cpg = TurningCPG(sim, fly.name)
        eyes = EyeRenderer(sim, fly.name, scene=Scene(checker_size=2.0, ground_rgb=((0, 0, 0), (1, 1, 1))))
        net = RetinotopicNetwork(sim, fly.name, motion_pathway(), dt=20 * float(sim.timestep), substeps=2, gain=40.0)
        omm = torch.zeros((n, 2, 721, 2), dtype=torch.float32, device=sim.device)

        def tick(eyes=eyes, cpg=cpg, net=net, omm=omm):
            eyes.render_into(omm)
            net.update(omm, out=cpg.drive)
            cpg.step(20)

        eyes.render_into(omm)                              # (every other kernel of the chain has run before the capture)
        cpg.step(20)
        runs.append((sim, cpg, net, omm, tick))
    (s0, c0, n0, omm0, eager), (s1, c1, n1, omm1, captured) = runs
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                              # captured before this network has ever been updated
        captured()
    drives = []
    for k in range(8):
        g.replay()
        eager()
        torch.cuda.synchronize()
        assert torch.equal(omm0, omm1), k
        assert torch.equal(c0.drive, c1.drive) and torch.equal(c0.phase, c1.phase) and torch.equal(c0.magnitude, c1.magnitude), k
        for name in VIEWS:
            if name != "drive":
                assert torch.equal(getattr(n0, name), getattr(n1, name)), (k, name)
        for key in keys:
            assert torch.equal(s0.field(key), s1.field(key)), (k, key)
        drives.append(c1.drive.clone())
    assert not torch.equal(drives[0], drives[-1]) and bool(torch.isfinite(s1.field("qpos")).all())
    assert bool((n1.fresh == 0).all()) and bool((n1.pooled[:, :, 1:] > 0).any())
    n0.close(); n1.close(); c0.close(); c1.close()


def test_refusals_leave_everything_untouched(torch_mod):
    torch = torch_mod
    from flygym_amd import _native
    from flygym_amd.sensors import FlatNetwork, Retina, RetinotopicNetwork, _VisnetParams, motion_pathway

    n = 3
    sim, fly = _plain_batch(n)
    dev = sim.device
    network, flat, table, retina = _case("ragged", 1)
    live = RetinotopicNetwork(sim, fly.name, network, dt=spec.DT, retina=retina, neighbours=table, **spec.PARAMS)
    C = flat.n_types
    omm = torch.zeros((n, 2, 721, 2), dtype=torch.float32, device=dev)
    out = torch.zeros((n, 2), dtype=torch.float32, device=dev)
    for name in ("v", "pooled", "signal", "drive"):
        getattr(live, name).fill_(-5.0)
    live.sums.fill_(-5)
    before = {key: sim.field(key).clone() for key in ("qpos", "ctrl", "time")}
    bad = [dict(omm=omm[:-1]), dict(omm=omm[:, :1]), dict(omm=torch.zeros((n, 2, 720, 2), device=dev)), dict(omm=omm.double()),
           dict(omm=omm.cpu()), dict(omm=torch.zeros((n, 2, 2, 721), device=dev).transpose(2, 3)), dict(omm=omm.cpu().numpy()),
           dict(omm=omm, base=out[:-1]), dict(omm=omm, base=out.double()), dict(omm=omm, base=out.cpu()), dict(omm=omm, base=1.0),
           dict(omm=omm, base=torch.zeros((2, n), device=dev).t()), dict(omm=omm, out=out[:-1]), dict(omm=omm, out=out.cpu()),
           dict(omm=omm, out=torch.zeros((2, n), device=dev).t()), dict(omm=omm, out=out.double())]
    for kw in bad:
        with pytest.raises(ValueError):
            live.update(**kw)
    with pytest.raises(ValueError, match="shape"):
        live.reset(np.zeros(n - 1, dtype=bool))
    make = lambda **kw: RetinotopicNetwork(sim, fly.name, **{**dict(network=network, dt=spec.DT, retina=retina, neighbours=table), **spec.PARAMS, **kw})
    with pytest.raises(ValueError, match="1024"):
        make(retina=Retina(id_map=np.arange(1, 1026, dtype=np.int16).reshape(25, 41)), neighbours=np.zeros((1, 1025), dtype=np.int32))
    with pytest.raises(ValueError, match="substeps"):
        make(substeps=9)
    with pytest.raises(ValueError, match="substeps"):
        make(substeps=0)
    with pytest.raises(ValueError, match="neighbours"):
        make(neighbours=table[:, :, :700])
    with pytest.raises(ValueError, match="neighbours"):
        make(neighbours=np.zeros((20, 721), dtype=np.int32))
    with pytest.raises(ValueError, match="neighbours"):
        make(neighbours=table.astype(np.float64))
    with pytest.raises(ValueError, match="outside"):
        make(neighbours=np.full((19, 721), 721, dtype=np.int32))
    with pytest.raises(ValueError, match="row outside"):
        make(neighbours=table[:, :7])
    with pytest.raises(ValueError, match="cells"):
        make(network=_case("widest", 1)[0], retina=spec.retina("square"), neighbours=np.zeros((1, 1024), dtype=np.int32))
    with pytest.raises(ValueError, match="positive"):
        make(dt=0.0)
    with pytest.raises(ValueError, match="unknown cell type"):
        make(network=dict(types=("a",), tau=dict(a=0.01), edges=[("a", "b", {0: 1.0})]))
    with pytest.raises(ValueError, match="no tau"):
        make(network=dict(types=("a", "b"), tau=dict(a=0.01)))
    with pytest.raises(ValueError, match="not finite"):
        make(network=FlatNetwork(("a",), [0.01], [np.nan], [[0, 0]], [0.0], np.zeros((0, 2), int), np.zeros((0, 2), int), []))
    with pytest.raises(ValueError):
        RetinotopicNetwork(sim, "nosuchfly", motion_pathway(), dt=spec.DT)
    # the limits at the C ABI: a null handle or a status, with a message that names the offending entry
    lib = _native.lib()
    assert ctypes.sizeof(_VisnetParams) == lib.nmf_visnet_params_size() == 44
    stream = sim._stream()
    types, edges, taps, tap_w = live.types, live.edges, live.taps, live.tap_w
    T, E, K = 19, len(edges), len(taps)

    def params(**kw):
        p = _VisnetParams.from_buffer_copy(live._params)
        for key, value in kw.items():
            setattr(p, key, value)
        return p

    def create(p, ty=types, nb=table, ed=edges, tp=taps, tw=tap_w):
        arrays = [None if a is None else np.ascontiguousarray(a) for a in (ty, nb, ed, tp, tw)]
        h = lib.nmf_visnet_create(sim._batch_h, None if p is None else ctypes.byref(p), *(None if a is None else a.ctypes.data for a in arrays))
        if h:
            lib.nmf_visnet_destroy(h)
        return h

    def changed(a, index, value):
        b = np.array(a)
        b[index] = value
        return b

    many_edges = np.zeros((513, 2), dtype=np.int32)
    many_taps, many_w = np.zeros((4097, 2), dtype=np.int32), np.zeros(4097, dtype=f32)
    wide = np.zeros((33, 5), dtype=f32); wide[:, 3] = 0.5
    for kw, message in [(dict(p=params(n_types=0)), "n_types must be in 1..32, got 0"),
                        (dict(p=params(n_types=33), ty=wide), "n_types must be in 1..32, got 33"),
                        (dict(p=params(n_omm=0)), "n_omm must be in 1..1024, got 0"),
                        (dict(p=params(n_omm=1025)), "n_omm must be in 1..1024, got 1025"),
                        (dict(p=params(n_types=25, n_omm=1024), ty=wide), "at most 24576 cells, got 25 x 1024 = 25600"),
                        (dict(p=params(n_table=0)), "n_table must be in 1..19, got 0"),
                        (dict(p=params(n_table=20)), "n_table must be in 1..19, got 20"),
                        (dict(p=params(n_edges=513), ed=many_edges), "n_edges must be in 0..512, got 513"),
                        (dict(p=params(n_edges=-1)), "n_edges must be in 0..512, got -1"),
                        (dict(p=params(n_taps=4097), tp=many_taps, tw=many_w), "n_taps must be in 0..4096, got 4097"),
                        (dict(p=params(substeps=0)), "substeps must be in 1..8, got 0"),
                        (dict(p=params(substeps=9)), "substeps must be in 1..8, got 9"),
                        (dict(p=params(), ed=None), "null edges / taps / tap weights"),
                        (dict(p=params(), tw=None), "null edges / taps / tap weights"),
                        (dict(p=params(gain=float("nan"))), "a parameter is not finite"),
                        (dict(p=params(), ty=changed(types, (2, 0), np.inf)), "bias of type 2 is not finite"),
                        (dict(p=params(), ty=changed(types, (4, 2), np.nan)), "in_w[1] of type 4 is not finite"),
                        (dict(p=params(), ty=changed(types, (1, 4), np.nan)), "steer_w of type 1 is not finite"),
                        (dict(p=params(), ty=changed(types, (3, 3), 0.0)), "a of type 3 must be in (0, 1]"),
                        (dict(p=params(), ty=changed(types, (0, 3), 1.5)), "a of type 0 must be in (0, 1]"),
                        (dict(p=params(), nb=changed(table, (1, 18, 720), 721)), "neighbours[1][18][720] = 721 is outside -1..720"),
                        (dict(p=params(), nb=changed(table, (0, 3, 5), -2)), "neighbours[0][3][5] = -2 is outside -1..720"),
                        (dict(p=params(), ed=changed(edges, (E - 1, 1), C)), f"edge {E - 1} = (0, {C}) is outside the network's {C} types"),
                        (dict(p=params(), ed=changed(edges, (0, 0), -1)), "edge 0 = (-1, 0) is outside the network's"),
                        (dict(p=params(), tp=changed(taps, (K - 1, 0), E)), f"tap {K - 1} belongs to edge {E}, outside the network's {E} edges"),
                        (dict(p=params(), tp=changed(taps, (3, 1), T)), f"tap 3 reads row {T}, outside the table's {T} rows"),
                        (dict(p=params(), tw=changed(tap_w, 9, np.nan)), "the weight of tap 9 is not finite"),
                        (dict(p=None), "null batch / params / types / neighbours"),
                        (dict(p=params(), nb=None), "null batch / params / types / neighbours")]:
        assert not create(**kw) and message in lib.nmf_last_error().decode(), (message, lib.nmf_last_error().decode())
    assert create(params(n_edges=0, n_taps=0), ed=None, tp=None, tw=None)                  # (a network without edges is valid)
    h = live._handle()
    for args, message in [((None, omm.data_ptr(), None, out.data_ptr()), "null handle"), ((h, None, None, out.data_ptr()), "null omm"),
                          ((h, omm.data_ptr(), None, None), "null drive"), ((h, omm.data_ptr() + 4, None, out.data_ptr()), "aligned"),
                          ((h, omm.data_ptr(), out.data_ptr() + 2, out.data_ptr()), "aligned")]:
        assert lib.nmf_visnet_update(*args, stream) != 0 and message in lib.nmf_last_error().decode(), message
    assert lib.nmf_visnet_reset(None, None, stream) != 0 and "null handle" in lib.nmf_last_error().decode()
    assert not lib.nmf_visnet_field_ptr(h, 6, None) and "no such field" in lib.nmf_last_error().decode()
    assert not lib.nmf_visnet_field_ptr(None, 0, None) and "null handle" in lib.nmf_last_error().decode()
    # the live handle and the batch read as before, and a valid creation still works
    torch.cuda.synchronize()
    for name in ("v", "pooled", "signal", "drive"):
        assert bool((getattr(live, name) == -5).all()), name
    assert bool((live.sums == -5).all()) and bool((out == 0).all()) and bool((live.fresh == 1).all())
    for key, value in before.items():
        assert torch.equal(sim.field(key), value), key
    with make() as again:
        frames = torch.as_tensor(np.array(spec.readings(721)[0]), device=dev)
        state, want = _reference("ragged", 1)[0]
        for net in (again, live):
            drive = net.update(frames)
            torch.cuda.synchronize()
            _assert_equal_bits("after the refusals", net, drive, state, want)
    live.close()
    assert live.drive is None and live.v is None
    with pytest.raises(RuntimeError, match="closed"):
        live.update(omm)


def test_a_multi_fly_world_resolves_to_the_flys_batch(torch_mod):
    torch = torch_mod
    from flygym_amd.sensors import RetinotopicNetwork

    sim, fly = _plain_batch(3)

    class Several:                                         # what RetinotopicNetwork asks of a MultiFlyHIPSimulation
        def for_fly(self, name):
            assert name == fly.name
            return sim

    network, flat, table, retina = _case("ring", 2)
    frames = torch.as_tensor(np.array(spec.readings(7)[0]), device=sim.device)
    with RetinotopicNetwork(Several(), fly.name, network, dt=spec.DT, retina=retina, neighbours=table, substeps=2, **spec.PARAMS) as net:
        assert net.sim is sim
        drive = net.update(frames)
        torch.cuda.synchronize()
        state, want = _reference("ring", 2)[0]
        _assert_equal_bits("for_fly", net, drive, state, want)
