"""Plume navigation on the GPU (``flygym_amd/csrc/nmf_navigator.hip``, ``flygym_amd.controllers.PlumeNavigator``) against its numpy
specification ``tests/navigator_spec.py``.

The inputs are synthetic except in the captured-graph test: after ``sim.reset()`` the tests write chosen quaternions into the
zero-copy view ``seg_xquat`` of the batch and pass odor and wind tensors directly; nothing steps in between, so the inputs are
exactly known.  The comparison rule: every view equals the specification's bit for bit after every update (floats compared as
bytes).  ``tests/test_navigator_cpu.py`` asserts that the inputs used here take every transition of the state machine."""
import ctypes
import functools

import numpy as np
import pytest

import navigator_spec as spec

pytestmark = pytest.mark.gpu

FIELDS = spec.FIELDS
KEYS = ("qpos", "qvel", "ctrl", "seg_xpos", "seg_xquat", "sensordata", "time")
N_DIMS, ODOR_DIM = 2, 1
RATES = dict(stop_rate=(4 * 0.78, 4 * -0.61), walk_rate=(4 * 0.29, 4 * 0.41), turn_rate=4 * 1.33, p_up=(0.5, 0.15), p_up_bounds=(0.05, 0.95),
             turn_drive=(0.4, 1.2))


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


def _navigator(sim, fly, **over):
    """A navigator with the parity settings of the specification module (``spec.PARITY``)."""
    from flygym_amd.controllers import PlumeNavigator

    kw = dict(threshold=0.1, seed=spec.SEED, first_world=spec.first_world(sim.n_worlds), odor_dim=ODOR_DIM, **spec.PARITY_TIMES, **RATES)
    return PlumeNavigator(sim, fly.name, **{**kw, **over})


def _root_quat_view(sim, nav):
    return sim.field("seg_xquat").view(sim.n_worlds, sim.model.nseg, 4)[:, nav.root_seg]


def _clone(nav, drive=None):
    return {name: (getattr(nav, name) if name != "drive" or drive is None else drive).clone() for name in FIELDS}


def _numpy(torch, clones):
    """A list of per-update dicts of device tensors -> one dict of stacked numpy arrays (T, n, ...)."""
    torch.cuda.synchronize()
    got = {name: torch.stack([c[name] for c in clones]).cpu().numpy() for name in FIELDS}
    got["ticks"] = got["ticks"].view(np.uint32)                                    # (the view shows the uint32 counter as int32)
    return got


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


@functools.lru_cache(maxsize=None)
def _gpu_run(n, T, layout):
    """T updates of an n-world batch on the device from the specification module's inputs; every view after every update, as numpy.
    layout: "rows" one wind row per world, "shared" the wind row of world n - 1 as the one shared row, "repeated" that row n times.
    The "rows" run writes its drive into a caller's tensor, the others into the navigator's own."""
    import torch

    sim, fly = _batch(n)
    sim.reset()
    dev = sim.device
    odor, wind, quat = (torch.as_tensor(np.array(a), device=dev) for a in spec.input_run(n, T))
    if layout == "shared":
        wind = wind[:, -1:, :].contiguous()
    elif layout == "repeated":
        wind = wind[:, -1:, :].expand(T, n, 2).contiguous()
    out = torch.full((n, 2), -7.0, dtype=torch.float32, device=dev) if layout == "rows" else None
    clones = []
    with _navigator(sim, fly) as nav:
        assert spec.Params.from_struct(nav._params) == spec.PARITY and nav.constants["turn_ticks"] == spec.PARITY.turn_ticks
        assert tuple(nav.state.shape) == (n,) and tuple(nav.drive.shape) == (n, 2) and nav.ticks.dtype == torch.int32
        assert not bool(nav.state.any()) and torch.equal(nav.drive, torch.ones_like(nav.drive))
        root = _root_quat_view(sim, nav)
        for k in range(T):
            root.copy_(quat[k])
            drive = nav.update(odor[k], wind[k], out=out)
            assert drive is (nav.drive if out is None else out)
            clones.append(_clone(nav, out))
        got = _numpy(torch, clones)
        if out is not None:                                                         # the navigator's own drive was never written
            assert torch.equal(nav.drive, torch.ones_like(nav.drive))
    for a in got.values():
        a.setflags(write=False)
    return got


@pytest.mark.parametrize("layout", ["rows", "shared", "repeated"])
@pytest.mark.parametrize("n,T", spec.CASES)
def test_parity_with_the_specification(torch_mod, n, T, layout):
    """1, 65 and 257 worlds (one lane past a wave and past a workgroup), 300, 120 and 60 updates of random antennal readings, winds
    and tilted attitudes with NaN and +-Inf among them, the second of two odor dimensions read; every view after every update
    equals the specification's bytes.  One wind row per world, one shared row, and that row repeated per world: the last two get
    the same values and give identical results."""
    snaps, cover = spec.reference_run(n, T, layout != "rows")
    got = _gpu_run(n, T, layout)
    _assert_same(got, _stacked(snaps), (n, T, layout))
    if layout == "repeated":
        shared = _gpu_run(n, T, "shared")
        assert all(got[name].tobytes() == shared[name].tobytes() for name in FIELDS)
    assert min(cover[k] for k in cover) >= 3 and (got["ticks"][-1] == T).all()
    print(f"navigator parity, {n} worlds x {T} updates, wind {layout}: all views bit for bit; {cover}")


def test_a_world_does_not_depend_on_its_place_in_the_batch(torch_mod):
    """World n - 1 of the 1-, 65- and 257-world batches has the same global index (first_world = 257 - n) and the same inputs: its
    state is byte-identical after every one of the updates the runs share."""
    runs = [(_gpu_run(n, T, "rows"), T) for n, T in spec.CASES]
    for name in FIELDS:
        for other, T in runs[1:]:
            assert runs[0][0][name][:T, 0].tobytes() == other[name][:, -1].tobytes(), name
    alone = runs[0][0]
    assert len(np.unique(alone["state"][:60, 0])) == 4 and alone["encounters"][59, 0] >= 3
    # and it does depend on the global index: the same inputs at another first_world decide otherwise
    torch = torch_mod
    sim, fly = _batch(1)
    odor, wind, quat = (torch.as_tensor(np.array(a), device=sim.device) for a in spec.input_run(1, 60))
    with _navigator(sim, fly, first_world=3) as nav:
        states = []
        for k in range(60):
            _root_quat_view(sim, nav).copy_(quat[k])
            nav.update(odor[k], wind[k])
            states.append(nav.state.clone())
        torch.cuda.synchronize()
        assert not np.array_equal(torch.stack(states).cpu().numpy(), alone["state"][:60])


def test_masked_reset(torch_mod):
    """65 worlds; after 20 updates the odd ones are reset and everything runs 25 more.  The masked worlds restart at WALK, tick 0
    and the walk drive and follow a specification reset the same way; the others are byte-identical to an undisturbed twin."""
    torch = torch_mod
    n, T0, T1 = 65, 20, 25
    sim, fly = _batch(n)
    sim.reset()
    odor, wind, quat = (torch.as_tensor(np.array(a), device=sim.device) for a in spec.input_run(n, T0 + T1))
    mask = np.arange(n) % 2 == 1
    st = spec.State(n, spec.PARITY, seed=spec.SEED, first_world=spec.first_world(n))
    snaps = []
    with _navigator(sim, fly) as nav, _navigator(sim, fly) as twin:
        root = _root_quat_view(sim, nav)
        clones, twins = [], []

        def run(k0, k1):
            for k in range(k0, k1):
                root.copy_(quat[k])
                nav.update(odor[k], wind[k]); twin.update(odor[k], wind[k])
                clones.append(_clone(nav)); twins.append(_clone(twin))
                st.update(*(a[k] for a in spec.input_run(n, T0 + T1)), ODOR_DIM)
                snaps.append(st.snapshot())

        run(0, T0)
        before = _numpy(torch, clones[-1:])
        assert before["state"][0, mask].any() and before["k_stop"][0, mask].any() and (before["ticks"] == T0).all()
        nav.reset(torch.as_tensor(mask))
        st.reset(mask)
        after = _numpy(torch, [_clone(nav)])
        for name in FIELDS[:-1]:
            assert not after[name][0, mask].any(), name
            assert after[name][0, ~mask].tobytes() == before[name][0, ~mask].tobytes(), name
        assert np.array_equal(after["drive"][0, mask], np.ones((int(mask.sum()), 2), dtype=np.float32))
        assert after["drive"][0, ~mask].tobytes() == before["drive"][0, ~mask].tobytes()
        run(T0, T0 + T1)
        got, undisturbed = _numpy(torch, clones), _numpy(torch, twins)
        _assert_same(got, _stacked(snaps), "masked reset")
        assert (got["ticks"][-1, mask] == T1).all() and (got["ticks"][-1, ~mask] == T0 + T1).all()
        for name in FIELDS:
            assert got[name][:, ~mask].tobytes() == undisturbed[name][:, ~mask].tobytes(), name
        assert got["state"][T0:, mask].tobytes() != undisturbed["state"][T0:, mask].tobytes()
        # a reset of every world, from a numpy mask and from none
        nav.reset(np.ones(n, dtype=bool)); twin.reset()
        both = _numpy(torch, [_clone(nav), _clone(twin)])
        assert not any(both[name].any() for name in FIELDS[:-1]) and (both["drive"] == 1).all()


def test_one_control_tick_is_one_captured_graph(torch_mod):
    """Two settled 11-world batches with identical plumes and seeds.  One tick is ``plume.advance()``, the readings into a fixed
    buffer, ``nav.update(buf, plume.wind, out=cpg.drive)`` and ``cpg.step(20)``: eight eager ticks on one batch against one capture
    replayed eight times on the other (one stream, one linear chain).  All navigator views, the wind and the batch fields are
    identical, and the specification, fed the readings, winds and quaternions recorded before each eager update, agrees bit for
    bit.  The rates are high enough that the specification changes state in at least 3 of the 11 worlds."""
    torch = torch_mod
    from flygym_amd.controllers import TurningCPG
    from flygym_amd.sensors import OdorPlume

    n, ticks, steps = 11, 8, 20
    sides = []
    for copy in (1, 2):
        sim, fly = _batch(n, copy=copy)
        sim.reset()
        sim.warmup()
        tick_s = steps * sim.timestep
        plume = OdorPlume(sim, fly.name, grid=(32, 48), cell_size=0.25, origin=(-4.0, -4.0), source=(2.5, 0.0, 1.0, 1.0), mean_wind=(-60.0, 0.0),
                          wind_tau=0.5, wind_sigma=60.0, diffusivity=1.0, tick_s=tick_s, seed=5)
        cpg = TurningCPG(sim, fly.name, table_steps=32)
        buf = torch.zeros((n, 1, 4), dtype=torch.float32, device=sim.device)
        plume.advance(60)
        plume.advance()                                                            # one whole tick without the navigator: every
        plume.get_odor_intensities(out=buf)                                        # other kernel of the chain has run before the capture
        cpg.step(steps)
        nav = _navigator(sim, fly, tick_s=tick_s, threshold=1e-3, seed=9, first_world=0, odor_dim=0, stop_rate=(60.0, -20.0),
                         walk_rate=(150.0, 50.0), turn_rate=100.0, tau_stop=0.2, tau_walk=0.52, tau_freq=2.0, turn_duration=2 * tick_s)
        sides.append((sim, plume, cpg, nav, buf))
    torch.cuda.synchronize()
    (s0, pl0, c0, n0, b0), (s1, pl1, c1, n1, b1) = sides
    assert n0.constants["turn_ticks"] == 2
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pl1.advance()
        pl1.get_odor_intensities(out=b1)
        n1.update(b1, pl1.wind, out=c1.drive)
        c1.step(steps)
    assert not bool(n1.ticks.any())                                                # (the capture itself ran nothing)
    st = spec.State(n, spec.Params.from_struct(n0._params), seed=9, first_world=0)
    changed = np.zeros(n, dtype=bool)
    for k in range(ticks):
        pl0.advance()
        pl0.get_odor_intensities(out=b0)
        torch.cuda.synchronize()
        recorded = (b0.cpu().numpy().copy(), pl0.wind.cpu().numpy().copy(), _root_quat_view(s0, n0).cpu().numpy().copy())
        n0.update(b0, pl0.wind, out=c0.drive)
        drive = c0.drive.clone()
        c0.step(steps)
        g.replay()
        before = st.state.copy()
        st.update(*recorded)
        changed |= st.state != before
        eager, replayed = _numpy(torch, [_clone(n0, drive)]), _numpy(torch, [_clone(n1, c1.drive)])
        _assert_same(eager, _stacked([st.snapshot()]), ("tick", k))
        for name in FIELDS:
            assert eager[name].tobytes() == replayed[name].tobytes(), (k, name)
        assert torch.equal(pl0.wind, pl1.wind) and torch.equal(b0, b1), k
        for key in KEYS:
            assert torch.equal(s0.field(key), s1.field(key)), (k, key)
    print(f"navigator in the captured tick, {n} worlds x {ticks} ticks: state changed in {int(changed.sum())} worlds, "
          f"{int(st.encounters.sum())} encounters, largest reading {float(b0.max()):.3g}, states now {st.state.tolist()}")
    assert int(changed.sum()) >= 3 and (eager["ticks"] == ticks).all()
    assert torch.equal(n0.drive, torch.ones_like(n0.drive))                        # (out= was given: the own drive stays)
    for _, plume, cpg, nav, _ in sides:
        nav.close(); cpg.close(); plume.close()


def test_refusals_leave_the_state_untouched(torch_mod):
    """Every refused creation and update raises / returns its message and leaks nothing (a following valid creation works); a live
    navigator's views read the same before and after each refusal; a closed navigator and wrong shapes, dtypes and devices are
    refused in Python."""
    torch = torch_mod
    from flygym_amd import _native
    from flygym_amd.controllers import PlumeNavigator, _NavigatorParams

    lib = _native.lib()
    n = 11
    sim, fly = _batch(n)
    sim.reset()
    dev = sim.device
    odor, wind, quat = (torch.as_tensor(np.array(a), device=dev) for a in spec.input_run(n, 12))
    live = _navigator(sim, fly, first_world=0)
    for k in range(12):
        _root_quat_view(sim, live).copy_(quat[k])
        live.update(odor[k], wind[k])
    before = _numpy(torch, [_clone(live)])
    assert before["state"].any() and before["k_stop"].any() and (before["ticks"] == 12).all()

    def unchanged():
        now = _numpy(torch, [_clone(live)])
        assert all(now[name].tobytes() == before[name].tobytes() for name in FIELDS)

    nseg = sim.model.nseg

    def create(**over):
        p = _NavigatorParams.from_buffer_copy(live._params)
        for key, value in over.items():
            if isinstance(value, tuple):
                getattr(p, key)[value[0]] = value[1]
            else:
                setattr(p, key, value)
        return lib.nmf_navigator_create(sim._batch_h, ctypes.byref(p))

    nan, inf = float("nan"), float("inf")
    refusals = [(dict(lambda_turn=nan), b"not finite"), (dict(dt=inf), b"not finite"), (dict(threshold=nan), b"not finite"),
                (dict(up_gain=-inf), b"not finite"), (dict(turn_drive=(1, nan)), b"not finite"), (dict(walk_drive=(0, inf)), b"not finite"),
                (dict(threshold=-0.5), b"threshold"),
                (dict(decay_stop=1.5), b"decay"), (dict(decay_walk=-0.1), b"decay"), (dict(decay_freq=2.0), b"decay"),
                (dict(p_up_min=0.8, p_up_max=0.2), b"p_up_min"), (dict(p_up_max=1.5), b"p_up_min"), (dict(p_up_min=-0.1), b"p_up_min"),
                (dict(turn_ticks=0), b"turn_ticks"), (dict(turn_ticks=65536), b"turn_ticks"), (dict(turn_ticks=-2), b"turn_ticks"),
                (dict(root_seg=nseg), b"root_seg"), (dict(root_seg=-1), b"root_seg"),
                (dict(odor_dim=8), b"odor_dim"), (dict(odor_dim=-1), b"odor_dim"), (dict(first_world=-1), b"first_world")]
    for over, text in refusals:
        assert not create(**over) and text in lib.nmf_last_error(), (over, lib.nmf_last_error())
        unchanged()
    assert not lib.nmf_navigator_create(sim._batch_h, None) and b"null" in lib.nmf_last_error()
    assert not lib.nmf_navigator_create(None, ctypes.byref(live._params)) and b"null" in lib.nmf_last_error()
    # the Python class raises NativeError with the library's message, or ValueError before it gets there
    with pytest.raises(_native.NativeError, match="threshold must not be negative"):
        _navigator(sim, fly, threshold=-1.0)
    with pytest.raises(_native.NativeError, match="odor_dim must be in 0..7"):
        _navigator(sim, fly, odor_dim=8)
    with pytest.raises(_native.NativeError, match="p_up_min"):
        _navigator(sim, fly, p_up_bounds=(0.9, 0.1))
    with pytest.raises(_native.NativeError, match="not finite"):
        _navigator(sim, fly, turn_rate=nan)
    with pytest.raises(ValueError, match="turn_duration"):
        _navigator(sim, fly, turn_duration=0.0)
    with pytest.raises(ValueError, match="tau_stop"):
        _navigator(sim, fly, tau_stop=0.0)
    with pytest.raises(ValueError, match="turn_drive"):
        _navigator(sim, fly, turn_drive=(1.0, 2.0, 3.0))
    unchanged()

    # refused updates, at the C ABI
    h, stream = live._handle(), sim._stream()
    o, w = odor[0], wind[0]
    out = torch.zeros((n, 2), dtype=torch.float32, device=dev)
    calls = [((h, None, N_DIMS, w.data_ptr(), n, None, stream), b"null odor"),
             ((h, o.data_ptr(), N_DIMS, None, n, None, stream), b"null wind"),
             ((h, o.data_ptr(), 1, w.data_ptr(), n, None, stream), b"dimension"),
             ((h, o.data_ptr(), 0, w.data_ptr(), n, None, stream), b"dimension"),
             ((h, o.data_ptr(), N_DIMS, w.data_ptr(), 2, None, stream), b"wind_rows"),
             ((h, o.data_ptr(), N_DIMS, w.data_ptr(), 0, None, stream), b"wind_rows"),
             ((h, o.data_ptr(), N_DIMS, w.data_ptr(), n + 1, None, stream), b"wind_rows"),
             ((h, o.data_ptr() + 4, N_DIMS, w.data_ptr(), n, None, stream), b"aligned"),
             ((h, o.data_ptr(), N_DIMS, w.data_ptr(), n, out.data_ptr() + 4, stream), b"aligned"),
             ((None, o.data_ptr(), N_DIMS, w.data_ptr(), n, None, stream), b"null navigator")]
    for args, text in calls:
        assert lib.nmf_navigator_update(*args) != 0 and text in lib.nmf_last_error(), (args, lib.nmf_last_error())
        unchanged()
    assert not bool(out.any())
    assert lib.nmf_navigator_reset(None, None, None) != 0 and b"null navigator" in lib.nmf_last_error()
    assert not lib.nmf_navigator_field_ptr(h, 9, None) and b"no such field" in lib.nmf_last_error()
    assert not lib.nmf_navigator_field_ptr(h, -1, None) and b"no such field" in lib.nmf_last_error()

    # wrong shapes, dtypes and devices, in Python
    bad_updates = [(dict(odor=o[:, :, :3].contiguous()), "odor"), (dict(odor=o[:, :1].contiguous()), "dimension"), (dict(odor=o.double()), "odor"),
                   (dict(odor=o.cpu()), "odor"), (dict(odor=o[:5].contiguous()), "odor"), (dict(odor=o.cpu().numpy()), "odor"),
                   (dict(odor=o.transpose(1, 2)), "odor"),
                   (dict(wind=w[:, :1].contiguous()), "wind"), (dict(wind=w.double()), "wind"), (dict(wind=w.cpu()), "wind"),
                   (dict(wind=w[:2].contiguous()), "wind"), (dict(wind=torch.zeros((n, 4), device=dev)[:, :2]), "wind"),
                   (dict(out=torch.zeros((n, 3), device=dev)), "out"), (dict(out=torch.zeros((n, 2), dtype=torch.float64, device=dev)), "out"),
                   (dict(out=torch.zeros((n, 2))), "out"), (dict(out=torch.zeros((n, 4), device=dev)[:, :2]), "out")]
    for over, text in bad_updates:
        with pytest.raises(ValueError, match=text):
            live.update(**{**dict(odor=o, wind=w), **over})
    with pytest.raises(ValueError, match="reset mask"):
        live.reset(np.ones(n + 1, dtype=bool))
    unchanged()

    # a following valid creation works; the shapes of a shared wind
    h2 = create()
    assert h2
    width = ctypes.c_int32(0)
    assert lib.nmf_navigator_field_ptr(h2, 8, ctypes.byref(width)) and width.value == 2
    assert lib.nmf_navigator_field_ptr(h2, 0, ctypes.byref(width)) and width.value == 1
    assert lib.nmf_navigator_update(h2, o.data_ptr(), N_DIMS, w.data_ptr(), n, None, stream) == 0
    lib.nmf_navigator_destroy(h2)
    with _navigator(sim, fly) as a, _navigator(sim, fly) as b, _navigator(sim, fly) as c:
        a.update(o, w[3]); b.update(o, w[3:4]); c.update(o, w[3:4].expand(n, 2).contiguous())
        torch.cuda.synchronize()
        assert int(a.ticks[0]) == 1
        for name in FIELDS:
            assert torch.equal(getattr(a, name), getattr(b, name)) and torch.equal(getattr(a, name), getattr(c, name))
    unchanged()
    live.close()
    for call in (lambda: live.update(o, w), live.reset):
        with pytest.raises(RuntimeError, match="closed"):
            call()
    assert live.state is None and live.drive is None and live.ticks is None
    with pytest.raises(ValueError, match="for_fly"):
        class Several:
            for_fly = None
        PlumeNavigator(Several(), fly.name, tick_s=0.05, threshold=0.1)
