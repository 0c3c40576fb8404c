"""Path integration on the GPU (``flygym_amd/csrc/nmf_odometry.hip``, ``flygym_amd.sensors.PathIntegrator``) against its numpy
specification ``tests/odometry_spec.py``.

The inputs are synthetic except in the captured-graph test: after ``sim.reset()`` the tests write chosen values into the zero-copy
views ``seg_xpos``, ``seg_xquat`` and ``sensordata`` of the batch and call ``update``; nothing steps in between, so the inputs are
exactly known.

The comparison rule: ``stride_total``, ``window_strides``, ``count`` and ``heading`` equal the specification's bit for bit;
``position`` and ``home`` lie within ``1e-7 x sum_k |dd_k|`` of it per world — 9.2e-8 is the absolute bound csrc/nmf_device.h
documents for ``sincos_bounded``, rounded up, and the float64 sums' rounding is orders below — with the sum taken over the
specification's own displacement increments since the world's reset.

The bar is a bound for ``position`` under a float32 sine and cosine: each component adds ``dd_k`` times a factor at most 9.2e-8
off.  ``home = -R(heading)^T position`` multiplies that position by the same factors once more, so with ``sincos_bounded`` its
deviation could reach ``2.6e-7 sum |dd|`` — measured with it on an MI355X: up to 1.157 of the bar, three of the nine parity cases
over it.  The kernel therefore evaluates the sine and cosine of the float32-rounded heading in float64 (``odo_sincos``, 2e-15), and
both estimates then sit orders below the bar, which is kept as it was set."""
import ctypes
import functools

import numpy as np
import pytest

import odometry_spec as spec

pytestmark = pytest.mark.gpu

WAVE_WORLDS, GROUP_WORLDS = 10, 40                       # csrc/nmf_odometry.hip: worlds per wave and per workgroup
SIZES = (1, WAVE_WORLDS + 1, GROUP_WORLDS + 1)
WINDOWS = (1, 3, 8)
THRESHOLDS = (0.0, 1.5, 3.0)                             # per leg position f, m, h
FIELDS = ("stride_total", "window_strides", "heading", "position", "home", "count")
KEYS = ("qpos", "qvel", "ctrl", "seg_xpos", "seg_xquat", "sensordata", "time")


@pytest.fixture
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch


@functools.lru_cache(maxsize=None)
def _batch(n, copy=0, sensors=True):
    from flygym_amd import HIPSimulation, make_model
    from flygym_amd.compose import FlatGroundWorld
    from flygym_amd.utils.math import Rotation3D

    fly, world, _ = make_model()
    if not sensors:
        world = FlatGroundWorld()
        world.add_fly(fly, (0, 0, 0.8), Rotation3D("quat", (1, 0, 0, 0)), add_ground_contact_sensors=False)
    sim = HIPSimulation(world, n_worlds=n, device=0)
    sim.set_leg_adhesion_states(fly.name, np.ones((n, 6), dtype=np.float32))
    sim.reset()
    return sim, fly


def _coefficients(seed=2):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(-0.4, 0.4, 6), rng.uniform(-1.0, 1.0, 6), [0.3, 1.5]])


def _integrator(sim, fly, window, **kw):
    from flygym_amd.sensors import PathIntegrator

    kw = dict(dict(contact_force_thresholds=THRESHOLDS, coefficients=_coefficients()), **kw)
    return PathIntegrator(sim, fly.name, window=window, **kw)


def _spec_state(pi):
    return spec.State(pi.n_worlds, pi.window, pi.contact_force_thresholds, _coefficients())


def _inputs(seed, k, n, nseg, root):
    """Inputs of update ``k`` for an ``n``-world batch (numpy float32, shaped like the batch's views).  World ``n - 1`` is the same
    world whatever ``n`` (its own random stream), the others are drawn per index.  Every segment gets a random position, the root
    a random tilted attitude; of the 36 contact states (found 0 / 1 / 2 with a force of 0.2 .. 4.5 against thresholds of 0, 1.5 and
    3) about a third are found > 0 with a force under a non-zero threshold."""
    def draw(rng, m):
        xpos = rng.uniform(-2.0, 2.0, (m, nseg, 3)).astype(np.float32)
        quat = np.zeros((m, nseg, 4), dtype=np.float32)
        quat[..., 0] = 1
        q = rng.normal(size=(m, 4)) * np.array([1.0, 0.25, 0.25, 1.0])          # tilted up to some 30 degrees, any yaw
        quat[:, root] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
        sd = rng.uniform(-1, 1, (m, 6, 16)).astype(np.float32)
        sd[..., 0] = rng.choice([0.0, 1.0, 1.0, 2.0], (m, 6))
        f = rng.normal(size=(m, 6, 3))
        sd[..., 1:4] = (f / np.linalg.norm(f, axis=-1, keepdims=True) * rng.uniform(0.2, 4.5, (m, 6, 1))).astype(np.float32)
        return xpos, quat, sd

    a = draw(np.random.default_rng([seed, k, 0]), n - 1)
    b = draw(np.random.default_rng([seed, k, 1]), 1)
    return tuple(np.concatenate([u, v]).reshape(n, -1) for u, v in zip(a, b))


def _write(torch, sim, inputs):
    for key, a in zip(("seg_xpos", "seg_xquat", "sensordata"), inputs):
        sim.field(key).copy_(torch.as_tensor(a, device=sim.device))


def _read(torch, pi):
    torch.cuda.synchronize()
    return {k: getattr(pi, k).cpu().numpy() for k in FIELDS}


def _compare(got, st, where="", worlds=slice(None)):
    """The comparison rule of this module's docstring.  The bitwise fields and ``position`` are asserted here; the largest deviation
    of ``home`` in units of its bar is returned (infinite where the bar is 0 and the deviation is not), and every test asserts it
    to be at most 1 as its last statement, so that a miss there does not hide the rest."""
    assert got["count"].dtype == np.int32 and got["heading"].dtype == np.float64 and got["position"].dtype == np.float64
    for name, want in (("stride_total", st.total), ("window_strides", st.win), ("count", st.count), ("heading", st.heading)):
        assert np.array_equal(got[name][worlds], want[worlds]), (where, name, got[name][worlds], want[worlds])
    bar = 1e-7 * st.moved[worlds][:, None]
    dev = np.abs(got["position"][worlds] - st.position[worlds])
    assert (dev <= bar).all(), (where, "position", float((dev - bar).max()), dev, bar)
    dev = np.abs(got["home"][worlds] - st.home[worlds])
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(dev > 0, dev / bar, 0.0).max())


@functools.lru_cache(maxsize=None)
def _reference_run(n, window, nseg, root, tips, seed=7):
    """The specification's states after each of the 2 window + 3 updates of an n-world batch (computed once, shared)."""
    by_pos = dict(zip("fmh", THRESHOLDS))
    st = spec.State(n, window, [by_pos[p] for p in "fmhfmh"], _coefficients())
    snaps = []
    for k in range(2 * window + 3):
        st.update(*_inputs(seed, k, n, nseg, root), root, tips)
        snaps.append({key: np.copy(getattr(st, key)) for key in ("total", "win", "count", "heading", "position", "home", "moved", "cprev")})
    return snaps


class _Snap:
    def __init__(self, d):
        self.__dict__.update(d)


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("n", SIZES)
def test_parity_with_the_specification(torch_mod, n, window):
    """1, 11 and 41 worlds (one more than a wave's and than a workgroup's), windows of 1, 3 and 8, 2 window + 3 updates each so that
    every ring slot is overwritten at least once; fresh random poses, attitudes and contact states before every update, compared
    by the module's rule after every update."""
    torch = torch_mod
    sim, fly = _batch(n)
    worst, contacts, strides = 0.0, 0, 0
    with _integrator(sim, fly, window) as pi:
        assert pi.contact_force_thresholds.tolist() == [0.0, 1.5, 3.0, 0.0, 1.5, 3.0]
        snaps = _reference_run(n, window, sim.model.nseg, pi.root_seg, tuple(pi.tip_seg.tolist()))
        assert tuple(pi.stride_total.shape) == (n, 6) and tuple(pi.heading.shape) == (n,) and tuple(pi.home.shape) == (n, 2)
        assert tuple(pi.coefficients.shape) == (14,) and np.array_equal(pi.coefficients.cpu().numpy(), _coefficients())
        assert not bool(pi.count.any()) and not bool(pi.position.any())
        for k, snap in enumerate(snaps):
            _write(torch, sim, _inputs(7, k, n, sim.model.nseg, pi.root_seg))
            pi.update()
            worst = max(worst, _compare(_read(torch, pi), _Snap(snap), where=(n, window, k)))
            contacts += int(snap["cprev"].sum())
        strides = int((snaps[-1]["total"] != 0).sum())
        assert np.isfinite(snaps[-1]["position"]).all() and (snaps[-1]["moved"] > 0).all()
        assert (np.abs(snaps[-1]["heading"]) <= np.pi).all()
    print(f"odometry parity, {n} worlds, window {window}: position within the bar, home at {worst:.3f} of it; {contacts} leg contacts, "
          f"{strides} of {6 * n} legs with a stride")
    assert 0 < contacts < 6 * n * len(snaps) and strides > 0                     # both contact states occur
    assert worst <= 1.0, ("home", worst)


@pytest.mark.parametrize("window", WINDOWS)
def test_a_world_does_not_depend_on_its_place_in_the_batch(torch_mod, window):
    """The same world's inputs at index 0 of a 1-world batch, at index 10 of the 11-world batch (alone in its wave) and at index 40
    of the 41-world batch (alone in its workgroup): every field, ``position`` and ``home`` included, is bit-identical after every
    update."""
    torch = torch_mod
    runs = [(n, *_batch(n)) for n in SIZES]
    pis = [_integrator(sim, fly, window) for _, sim, fly in runs]
    try:
        for k in range(2 * window + 3):
            states = []
            for (n, sim, _), pi in zip(runs, pis):
                _write(torch, sim, _inputs(7, k, n, sim.model.nseg, pi.root_seg))
                pi.update()
                states.append(_read(torch, pi))
            for name in FIELDS:
                for other in states[1:]:
                    assert states[0][name][0].tobytes() == other[name][-1].tobytes(), (window, k, name)
        assert np.abs(states[0]["position"]).max() > 0 and states[0]["count"][0] == 2 * window + 3
    finally:
        for pi in pis:
            pi.close()


def test_masked_reset_with_and_without_pose(torch_mod):
    """11 worlds, window 3.  After 5 updates the odd worlds are reset — first to a given pose, in a second round to zeros — and
    everything runs 9 more updates.  The masked worlds restart from the pose, prime again and match a specification reset the
    same way; the others are bit-identical to a twin integrator that was never disturbed."""
    torch = torch_mod
    n, window = WAVE_WORLDS + 1, 3
    sim, fly = _batch(n)
    mask = np.arange(n) % 2 == 1
    rng = np.random.default_rng(12)
    pose = np.concatenate([rng.uniform(-1.0, 1.0, (n, 2)), rng.uniform(-3.0, 3.0, (n, 1))], axis=1)
    worst_home = []
    for given in (pose, None):
        with _integrator(sim, fly, window) as pi, _integrator(sim, fly, window) as twin:
            st = _spec_state(pi)
            step = 0

            def run(updates):
                nonlocal step
                for _ in range(updates):
                    inputs = _inputs(21, step, n, sim.model.nseg, pi.root_seg)
                    _write(torch, sim, inputs)
                    pi.update(); twin.update()
                    st.update(*inputs, pi.root_seg, pi.tip_seg)
                    step += 1

            run(5)
            worst_home.append(_compare(_read(torch, pi), st, where="before the reset"))
            pi.reset(torch.as_tensor(mask) if given is None else mask, given)
            st.reset(mask, given)
            got = _read(torch, pi)
            assert not got["count"][mask].any() and not got["stride_total"][mask].any() and not got["window_strides"][mask].any()
            want_pose = np.zeros((n, 3)) if given is None else given
            assert np.array_equal(got["position"][mask], want_pose[mask, :2]) and np.array_equal(got["heading"][mask], want_pose[mask, 2])
            # (the home vector of a pose: |p| x the sine's and cosine's 9.2e-8, rounded up as in the module's rule)
            assert (np.abs(got["home"][mask] - st.home[mask]) <= 1e-7 * np.abs(want_pose[mask, :2]).sum(axis=1, keepdims=True)).all()
            run(1)
            got = _read(torch, pi)
            assert (got["count"][mask] == 1).all() and not got["stride_total"][mask].any()          # primed again: no stride yet
            assert (got["count"][~mask] == 6).all()
            run(8)
            got, undisturbed = _read(torch, pi), _read(torch, twin)
            worst = _compare(got, st, where="after the reset")
            worst_home.append(worst)
            assert (got["count"][mask] == 9).all() and got["stride_total"][mask].any()
            for name in FIELDS:
                assert got[name][~mask].tobytes() == undisturbed[name][~mask].tobytes(), name
                # (the window strides are differences of totals, the same again once the window lies after the reset)
                assert name == "window_strides" or got[name][mask].tobytes() != undisturbed[name][mask].tobytes(), name
            assert got["window_strides"][mask].tobytes() == undisturbed["window_strides"][mask].tobytes()
            print(f"odometry masked reset, pose {'given' if given is not None else 'zeros'}: position within the bar, home at {worst:.3f} of it")
    # a reset of every world
    with _integrator(sim, fly, window) as pi:
        _write(torch, sim, _inputs(21, 0, n, sim.model.nseg, pi.root_seg))
        pi.update(); pi.update()
        pi.reset()
        got = _read(torch, pi)
        assert not any(got[name].any() for name in FIELDS)
    assert max(worst_home) <= 1.0, ("home", worst_home)


def test_the_kernels_sine_and_cosine_are_float64(torch_mod):
    """``reset(pose=(1, 0, h))`` writes ``home = (-cos, sin)`` of the float32-rounded ``h`` — the products with 1 and 0 are exact —,
    so the views show the kernel's own sine and cosine.  984 headings over [-pi, pi]: random ones, and the float32 neighbours of
    every multiple of pi/4, where the reduction changes quadrant.  The bar is 1e-14: the polynomials leave out terms below 1e-15
    at pi/4 and round some dozen float64 operations on values up to 1 (1.1e-16 each), together 2e-15, times five."""
    torch = torch_mod
    n = GROUP_WORLDS + 1
    sim, fly = _batch(n)
    rng = np.random.default_rng(31)
    edges = np.arange(-4, 5) * (np.pi / 4)
    near = np.concatenate([np.nextafter(edges.astype(np.float32), np.float32(s)).astype(np.float64) for s in (-9, 9)] + [edges, [0.0]])
    near = np.clip(near, -np.pi, np.pi)
    h = np.concatenate([near, rng.uniform(-np.pi, np.pi, 24 * n - near.size)]).reshape(24, n)
    worst = 0.0
    with _integrator(sim, fly, 3) as pi:
        for row in h:
            pi.reset(pose=np.stack([np.ones(n), np.zeros(n), row], axis=1))
            got = _read(torch, pi)
            assert np.array_equal(got["heading"], row)                              # (wrap leaves [-pi, pi] as it is)
            x = row.astype(np.float32).astype(np.float64)
            worst = max(worst, float(np.abs(got["home"][:, 0] + np.cos(x)).max()), float(np.abs(got["home"][:, 1] - np.sin(x)).max()))
    print(f"odometry sine and cosine: largest deviation from numpy's {worst:.2e} over {h.size} headings (bar 1e-14)")
    assert worst <= 1e-14


def test_one_control_tick_is_one_captured_graph(torch_mod):
    """The engine's own walk: 11 settled worlds under a ``TurningCPG`` with unequal drives, 20 steps per tick, window 3.  Eight eager
    ticks (``cpg.step`` + ``update``) against a graph of the same two calls replayed eight times on a second batch: all integrator
    fields are bit-identical, and the specification, fed the poses and sensor values recorded after each eager tick's steps, matches
    by the module's rule.  The signs of the strides are reported, not barred."""
    torch = torch_mod
    from flygym_amd.controllers import TurningCPG

    n, window, ticks = WAVE_WORLDS + 1, 3, 8
    drives = np.stack([np.linspace(0.4, 1.2, n), np.linspace(1.2, 0.6, n)], axis=1).astype(np.float32)
    coef = np.concatenate([[0.2, 0.1, 0.15, -0.2, -0.1, -0.15], np.full(6, 1.0 / 6.0), [0.0, 0.0]])
    sides = []
    for copy in (1, 2):
        sim, fly = _batch(n, copy=copy)
        sim.reset()
        sim.warmup()
        cpg = TurningCPG(sim, fly.name, table_steps=32)
        cpg.set_drive(drives)
        pi = _integrator(sim, fly, window, coefficients=coef, contact_force_thresholds=(0.0, 0.0, 0.0))
        sides.append((sim, cpg, pi))
    torch.cuda.synchronize()
    (s0, c0, p0), (s1, c1, p1) = sides
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c1.step(20)
        p1.update()
    st = spec.State(n, window, np.zeros(6), coef)
    worst = 0.0
    for k in range(ticks):
        c0.step(20)
        torch.cuda.synchronize()
        recorded = [s0.field(key).cpu().numpy().copy() for key in ("seg_xpos", "seg_xquat", "sensordata")]
        p0.update()
        g.replay()
        st.update(*recorded, p0.root_seg, p0.tip_seg)
        eager, replayed = _read(torch, p0), _read(torch, p1)
        for name in FIELDS:
            assert eager[name].tobytes() == replayed[name].tobytes(), (k, name)
        for key in KEYS:
            assert torch.equal(s0.field(key), s1.field(key)), (k, key)
        worst = max(worst, _compare(eager, st, where=("tick", k)))
    assert (eager["count"] == ticks).all()
    assert all(np.isfinite(eager[name]).all() for name in FIELDS)
    total = eager["stride_total"]
    print(f"odometry on the engine's walk, {n} worlds x {ticks} ticks: position within the bar, home at {worst:.3f} of it; strides "
          f"positive {int((total > 0).sum())}, negative {int((total < 0).sum())}, zero {int((total == 0).sum())} of {total.size}; "
          f"mean estimated path {float(st.moved.mean()):.4f}, mean |heading| {float(np.abs(eager['heading']).mean()):.4f} rad")
    for _, cpg, pi in sides:
        pi.close(); cpg.close()
    assert worst <= 1.0, ("home", worst)


def test_refusals_leave_the_state_untouched(torch_mod):
    """Every refused creation raises ``NativeError`` with its message and leaks nothing (a following valid creation works); a live
    integrator's views read the same before and after each refusal; a closed integrator and wrong shapes are refused in Python."""
    torch = torch_mod
    from flygym_amd import _native
    from flygym_amd.sensors import PathIntegrator, _OdometryParams

    lib = _native.lib()
    n = WAVE_WORLDS + 1
    sim, fly = _batch(n)
    live = _integrator(sim, fly, 3)
    for k in range(5):
        _write(torch, sim, _inputs(3, k, n, sim.model.nseg, live.root_seg))
        live.update()
    before = _read(torch, live)
    assert before["position"].any() and before["stride_total"].any()
    coef_before = live.coefficients.cpu().numpy()

    def unchanged():
        now = _read(torch, live)
        assert all(now[name].tobytes() == before[name].tobytes() for name in FIELDS)
        assert np.array_equal(live.coefficients.cpu().numpy(), coef_before)

    nseg = sim.model.nseg
    good_coef = _coefficients()

    def create(coef=good_coef, **over):
        p = _OdometryParams.from_buffer_copy(live._params)
        for key, value in over.items():
            if isinstance(value, tuple):
                getattr(p, key)[value[0]] = value[1]
            else:
                setattr(p, key, value)
        c = None if coef is None else np.ascontiguousarray(coef, dtype=np.float64)
        return lib.nmf_odometry_create(sim._batch_h, ctypes.byref(p), None if c is None else c.ctypes.data)

    refusals = [(dict(window=0), b"window"), (dict(window=4097), b"window"), (dict(window=-3), b"window"),
                (dict(root_seg=nseg), b"root_seg"), (dict(root_seg=-1), b"root_seg"),
                (dict(tip_seg=(4, nseg)), b"tip_seg[4]"), (dict(tip_seg=(0, -1)), b"tip_seg[0]"),
                (dict(contact_force_threshold=(2, -1.0)), b"contact_force_threshold[2]"),
                (dict(contact_force_threshold=(5, float("nan"))), b"contact_force_threshold[5]"),
                (dict(contact_force_threshold=(0, float("inf"))), b"contact_force_threshold[0]")]
    for over, text in refusals:
        assert not create(**over) and text in lib.nmf_last_error(), (over, lib.nmf_last_error())
        unchanged()
    for value in (np.nan, np.inf):
        bad = good_coef.copy(); bad[9] = value
        assert not create(coef=bad) and b"coefficient 9" in lib.nmf_last_error()
        unchanged()
    assert not lib.nmf_odometry_create(sim._batch_h, None, None) and b"null" in lib.nmf_last_error()
    # the Python class raises NativeError with the library's message
    with pytest.raises(_native.NativeError, match="window must be in 1..4096"):
        _integrator(sim, fly, 0)
    with pytest.raises(_native.NativeError, match="window must be in 1..4096"):
        _integrator(sim, fly, 5000)
    with pytest.raises(_native.NativeError, match="contact_force_threshold"):
        _integrator(sim, fly, 3, contact_force_thresholds=(0.0, -2.0, 0.0))
    with pytest.raises(_native.NativeError, match="coefficient 13 is not finite"):
        _integrator(sim, fly, 3, coefficients=np.r_[np.zeros(13), np.inf])
    with pytest.raises(ValueError):
        _integrator(sim, fly, 3, coefficients=np.zeros(12))
    bare_sim, bare_fly = _batch(3, sensors=False)
    assert int(bare_sim.model["n_sensor"][0]) == 0
    with pytest.raises(_native.NativeError, match="no leg sensors"):
        _integrator(bare_sim, bare_fly, 3)
    unchanged()
    # wrong shapes
    with pytest.raises(ValueError, match="mask"):
        live.reset(np.ones(n + 1, dtype=bool))
    with pytest.raises(ValueError, match="pose"):
        live.reset(None, np.zeros((n, 2)))
    with pytest.raises(ValueError, match="pose"):
        live.reset(np.ones(n, dtype=bool), np.zeros(3))
    with pytest.raises(ValueError):
        live.set_coefficients(np.zeros(5), np.zeros(6))
    unchanged()
    # a following valid creation works, with NULL coefficients too
    h = create(coef=None)
    assert h
    width = ctypes.c_int32(0)
    assert lib.nmf_odometry_field_ptr(h, 6, ctypes.byref(width)) and width.value == 14
    assert not lib.nmf_odometry_field_ptr(h, 7, None) and b"no such field" in lib.nmf_last_error()
    assert lib.nmf_odometry_update(h, None) == 0
    lib.nmf_odometry_destroy(h)
    with _integrator(sim, fly, 3, coefficients=None) as fresh:
        fresh.update()
        fresh.set_coefficients(np.arange(6), -np.arange(6), 0.5, -0.5)
        torch.cuda.synchronize()
        assert fresh.coefficients.cpu().numpy().tolist() == [0, 1, 2, 3, 4, 5, 0, -1, -2, -3, -4, -5, 0.5, -0.5]
        assert int(fresh.count[0]) == 1
        truth = fresh.true_pose()
        assert tuple(truth.shape) == (n, 3) and truth.dtype == torch.float64 and bool(torch.isfinite(truth).all())
    unchanged()
    assert lib.nmf_odometry_update(None, None) != 0 and b"null integrator" in lib.nmf_last_error()
    assert lib.nmf_odometry_reset(None, None, None, None) != 0 and b"null integrator" in lib.nmf_last_error()
    live.close()
    for call in (live.update, live.reset, live.true_pose):
        with pytest.raises(RuntimeError, match="closed"):
            call()
    assert live.heading is None and live.coefficients is None
    with pytest.raises(ValueError, match="for_fly"):
        class Several:
            for_fly = None
        PathIntegrator(Several(), fly.name, window=3)
