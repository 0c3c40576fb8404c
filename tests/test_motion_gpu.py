"""Motion vision on the GPU (``flygym_amd/csrc/nmf_motion.hip``, ``flygym_amd.sensors.MotionDetectors``) against its numpy
specification ``tests/motion_spec.py``.

Every comparison with the specification is bit for bit: the kernel's flow sums are integers of terms rounded before they are added,
its quotients correctly rounded divisions of exact operands and its float32 rule is compiled without contraction or reassociation."""
import ctypes
import functools

import numpy as np
import pytest

import motion_spec as spec

pytestmark = pytest.mark.gpu

f32 = np.float32
N = 67                                       # prime: the last workgroup holds one world of two
DT = 0.002
PAIR_COUNTS = (0, 1, 63, 64, 65, 2070, 3072)
FIELDS = ("fast", "slow", "sums", "flow", "rotation", "translation")


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
def _plain_batch(n=N):
    """n worlds of the benchmark fly, never stepped: something for a MotionDetectors to belong to."""
    from flygym_amd import HIPSimulation, make_model

    fly, world, _ = make_model()
    return HIPSimulation(world, n_worlds=n, device=0), fly


@functools.lru_cache(maxsize=None)
def _walking_batch(n, copy=0):
    """n settled worlds with leg adhesion on (one per size and copy; a test that steps one asks for its own copy)."""
    from flygym_amd import HIPSimulation, make_model

    fly, world, _ = make_model()
    sim = HIPSimulation(world, n_worlds=n, device=0)
    sim.set_leg_adhesion_states(fly.name, np.ones((n, 6), dtype=np.float32))
    sim.warmup()
    return sim, fly


@functools.lru_cache(maxsize=None)
def _retina(n_omm):
    """The default retina for 721 ommatidia; otherwise one pixel per ommatidium."""
    from flygym_amd.sensors import Retina

    if n_omm == 721:
        return Retina()
    shape = (32, 32) if n_omm == 1024 else (1, n_omm)
    return Retina(id_map=np.arange(1, n_omm + 1, dtype=np.int16).reshape(shape))


@functools.lru_cache(maxsize=None)
def _pair_list(n_omm, n_pairs):
    """The default retina's own list for (721, 2070); otherwise a seeded random list (pairs may repeat) of random unit vectors that
    starts with (0, n_omm - 1) and (n_omm - 1, 0)."""
    if (n_omm, n_pairs) == (721, 2070):
        pairs, weights = _retina(721).motion_pairs()
    elif n_pairs == 0:
        pairs, weights = np.zeros((0, 2), dtype=np.int32), np.zeros((0, 2), dtype=f32)
    else:
        rng = np.random.default_rng(7 * n_omm + n_pairs)
        a = rng.integers(0, n_omm, n_pairs)
        b = (a + rng.integers(1, n_omm, n_pairs)) % n_omm                                  # never a itself
        pairs = np.stack([a, b], axis=-1).astype(np.int32)
        pairs[:2] = [(0, n_omm - 1), (n_omm - 1, 0)][:n_pairs]
        angle = rng.uniform(0, 2 * np.pi, n_pairs)
        weights = np.stack([np.cos(angle), np.sin(angle)], axis=-1).astype(f32)
    pairs.setflags(write=False); weights.setflags(write=False)
    return pairs, weights


@functools.lru_cache(maxsize=None)
def _readings(n_omm, ticks=5, n=N, seed=0):
    """(ticks, n, 2, n_omm, 2) float32, read-only; a reading sits in one channel, the other is 0.  World 0 sees the same frame at
    every tick, world 1 readings of up to 300 (correlator outputs far beyond the clamp), world 2 ommatidia that alternate between 0
    and 1 every tick (in a checkerboard), world 3 world 4's readings with every ommatidium pale and world 4 with none pale; the rest
    uniform in [0, 1) with a seeded pale mask."""
    rng = np.random.default_rng(500 * n_omm + seed)
    r = rng.random((ticks, n, 2, n_omm)).astype(f32)
    r[:, 0] = r[0, 0]
    r[:, 1] = (300.0 * rng.random((ticks, 2, n_omm))).astype(f32)
    r[:, 2] = ((np.arange(ticks)[:, None, None] + np.arange(n_omm)[None, None, :]) % 2).astype(f32)
    pale = np.broadcast_to(rng.random(n_omm) < 0.3, (n, 2, n_omm)).copy()
    if n > 4:
        r[:, 3] = r[:, 4]
        pale[3], pale[4] = True, False
    omm = np.zeros((ticks, n, 2, n_omm, 2), dtype=f32)
    omm[..., 0] = np.where(pale, 0, r)
    omm[..., 1] = np.where(pale, r, 0)
    omm.setflags(write=False)
    return omm


def _assert_equal_bits(label, motion, drive, state, want):
    got = {name: getattr(motion, name) for name in FIELDS}
    got["drive"] = drive
    ref = {**want, "fast": state["fast"], "slow": state["slow"]}
    for name, value in got.items():
        same = _bits(value.cpu().numpy()) == _bits(ref[name])
        assert same.all(), f"{label}: {name} differs in {int((~same).sum())} of {same.size} values, first at {np.argwhere(~same)[0].tolist()}"
    assert np.array_equal(motion.fresh.cpu().numpy() != 0, state["fresh"]), f"{label}: fresh"


@pytest.mark.parametrize("n_omm", [1, 2, 63, 64, 65, 721, 1024])
def test_the_kernel_equals_the_specification_bit_for_bit(torch_mod, n_omm):
    """Five consecutive updates per pair count: the first with the scalar base into the detectors' own drive, the second with a
    base tensor, the third — after a masked reset — with a base tensor into a view of a larger tensor, then two more."""
    torch = torch_mod
    from flygym_amd.sensors import MotionDetectors

    sim, fly = _plain_batch()
    retina = _retina(n_omm)
    assert retina.num_ommatidia == n_omm
    frames_host = _readings(n_omm)
    frames = torch.as_tensor(np.array(frames_host), device=sim.device)
    rng = np.random.default_rng(n_omm)
    base_host = rng.uniform(0.1, 1.5, (N, 2)).astype(f32)
    base = torch.as_tensor(base_host, device=sim.device)
    mask = np.zeros(N, dtype=bool)
    mask[[0, 5, 6, 33, N - 1]] = True
    seen = set()
    for n_pairs in PAIR_COUNTS if n_omm > 1 else (0,):                       # (one ommatidium has no partner)
        pairs, weights = _pair_list(n_omm, n_pairs)
        params = dict(gain=15.0, base=0.95, delta=0.7)
        with MotionDetectors(sim, fly.name, dt=DT, retina=retina, pairs=(pairs, weights), **params) as motion:
            assert motion.n_pairs == n_pairs and tuple(motion.fast.shape) == tuple(motion.slow.shape) == (N, 2, n_omm)
            assert tuple(motion.sums.shape) == tuple(motion.flow.shape) == (N, 2, 2) and motion.sums.dtype == torch.int32
            assert tuple(motion.rotation.shape) == tuple(motion.translation.shape) == (N,) and tuple(motion.drive.shape) == (N, 2)
            assert bool((motion.fresh == 1).all()) and bool((motion.drive == 1).all())
            state = spec.new_state(N, n_omm)
            big = torch.full((N + 2, 2), -3.0, dtype=torch.float32, device=sim.device)
            clamped = 0
            for k in range(5):
                label = f"n_omm {n_omm}, P {n_pairs}, update {k}"
                b, out = (None, None) if k in (0, 3, 4) else (base, None) if k == 1 else (base, big[1:N + 1])
                if k == 2:
                    motion.reset(mask)
                    spec.reset(state, mask)
                    torch.cuda.synchronize()
                    assert np.array_equal(motion.fresh.cpu().numpy() != 0, mask)
                drive = motion.update(frames[k], base=b, out=out)
                assert drive is (motion.drive if out is None else out)
                torch.cuda.synchronize()
                want = spec.update(state, frames_host[k], pairs, weights, dt=DT, front=motion.front_edge,
                                   **{**params, "base": 0.95 if b is None else base_host})
                _assert_equal_bits(label, motion, drive, state, want)
                clamped += int(want["clamped"][1].sum())
                seen.update(np.unique(want["drive"]).tolist())
                # what the special worlds promise
                still = np.full(2, 0.95, dtype=f32) if b is None else np.clip(base_host[0], f32(0.2), f32(1.2))
                assert not want["sums"][0].any() and not want["flow"][0].any() and np.array_equal(want["drive"][0], still)
                assert np.array_equal(want["sums"][3], want["sums"][4])                       # the pale channel reads as the yellow one
                if k == 2:
                    assert not want["sums"][mask].any()                                       # (a reset world's update is a first one)
                    assert bool((big[0] == -3).all()) and bool((big[-1] == -3).all())         # the view's neighbours stay
            if n_pairs >= 63:
                assert clamped > 0 and len(seen) > 20, (clamped, len(seen))                   # the clamp was reached; many drives
            if n_pairs >= 63 and n_omm >= 63 and (n_omm, n_pairs) != (721, 2070):             # (on the lattice's own list the terms cancel)
                assert np.abs(want["sums"][2]).max() > 0                                      # the alternating world correlates


def _between_the_eyes(sim, fly):
    names = [s.name for s in fly.get_bodysegs_order()]
    return sim.field("seg_xpos").reshape(sim.n_worlds, -1, 3)[:, [names.index("l_eye"), names.index("r_eye")]].mean(dim=1).cpu().numpy()


def _ring(torch, sim, eyes, angles_rad, count=8, ring_radius=8.0, radius=1.5):
    """(n, count, 4) float32 on the device: per world ``count`` spheres evenly on a horizontal ring about ``eyes[w]`` (the point
    between the eyes), at its height, the first at ``angles_rad[w]`` from the world's x axis (counter-clockwise seen from above)."""
    a = np.asarray(angles_rad, dtype=np.float64)[:, None] + 2 * np.pi * np.arange(count)[None, :] / count
    out = np.empty((sim.n_worlds, count, 4), dtype=f32)
    out[..., 0] = eyes[:, None, 0] + ring_radius * np.cos(a)
    out[..., 1] = eyes[:, None, 1] + ring_radius * np.sin(a)
    out[..., 2] = eyes[:, None, 2]
    out[..., 3] = radius
    return torch.as_tensor(out, device=sim.device)


def test_an_orbiting_scene_turns_the_drive_with_it(torch_mod):
    """Fixes the signs.  3 x 4 settled worlds that are never stepped; eight black spheres of radius 1.5 mm on a ring of radius 8 mm
    at eye height orbit the fly at +90 degrees/s (counter-clockwise seen from above), -90 degrees/s and not at all: eight objects at
    90 degrees/s pass at 2 Hz, near the detectors' peak.  300 ticks of 2 ms.  The rendered readings through the kernel equal the
    specification on the same readings bit for bit; the rotation signal averaged over the last 150 ticks is positive for the
    counter-clockwise group and negative for the clockwise one, the drive lower on the left and on the right; the still group has no
    flow at all and the base drive, exactly, at every tick."""
    torch = torch_mod
    from flygym_amd.sensors import MotionDetectors
    from flygym_amd.vision import EyeRenderer, Scene

    n, ticks = 12, 300
    sim, fly = _walking_batch(n)
    rate = np.deg2rad(np.repeat([90.0, -90.0, 0.0], 4))
    start = np.deg2rad(np.tile([0.0, 7.0, 19.0, 31.0], 3))                    # (the four worlds of a group differ in phase)
    eyes = EyeRenderer(sim, fly.name, scene=Scene(spheres=[(0, 0, -100, 1.5)] * 8, sphere_rgb=[(0, 0, 0)] * 8))
    omm = torch.zeros((n, 2, 721, 2), dtype=torch.float32, device=sim.device)
    centre = _between_the_eyes(sim, fly)
    with MotionDetectors(sim, fly.name, dt=DT) as motion:
        pairs, weights = motion.pairs, motion.weights
        state = spec.new_state(n, 721)
        rotation, drive = np.zeros((ticks, n)), np.zeros((ticks, n, 2))
        for k in range(ticks):
            eyes.set_spheres(_ring(torch, sim, centre, start + rate * (k * DT)))
            eyes.render_into(omm)
            d = motion.update(omm)
            torch.cuda.synchronize()
            want = spec.update(state, omm.cpu().numpy(), pairs, weights, dt=DT, front=motion.front_edge)
            _assert_equal_bits(f"tick {k}", motion, d, state, want)
            rotation[k], drive[k] = want["rotation"], want["drive"]
            assert not want["flow"][8:].any() and (want["drive"][8:] == 1).all(), k
        assert int(want["clamped"].sum()) == 0
    rot = rotation[ticks // 2:].mean(axis=0).reshape(3, 4)
    drv = drive[ticks // 2:].mean(axis=0).reshape(3, 4, 2)
    for name, r, d in zip(("counter-clockwise", "clockwise", "still"), rot, drv):
        print(f"orbiting scene, {name}: rotation mean {r.mean():+.4e} (min {r.min():+.4e}, max {r.max():+.4e}), "
              f"drive (left, right) {d.mean(axis=0).round(4).tolist()}")
    assert (rot[0] > 0).all() and (rot[1] < 0).all() and (rot[2] == 0).all()
    assert (drv[0, :, 0] < drv[0, :, 1]).all() and (drv[1, :, 1] < drv[1, :, 0]).all()


def test_one_control_tick_is_one_captured_graph(torch_mod):
    """``update(omm, out=cpg.drive)`` + ``cpg.advance(20)`` + ``step_replay`` captured once on the batch's stream (a single chain),
    before the first update, and replayed seven times with new readings written in place: every field of the batch, the
    controller's state and the detectors' state equal the eager run's, and the last replay equals the specification."""
    torch = torch_mod
    from flygym_amd.controllers import TurningCPG
    from flygym_amd.sensors import MotionDetectors

    n = 16
    keys = ("qpos", "qvel", "ctrl", "qacc_warmstart", "seg_xpos", "seg_xquat", "site_xpos", "actuator_force", "sensordata", "time",
            "stats", "qacc", "stats_sum", "contact_geom", "act")
    runs = []
    for copy in (1, 2):
        sim, fly = _walking_batch(n, copy)
        cpg = TurningCPG(sim, fly.name)
        motion = MotionDetectors(sim, fly.name, dt=DT, gain=40.0)
        omm = torch.zeros((n, 2, 721, 2), dtype=torch.float32, device=sim.device)

        def tick(sim=sim, cpg=cpg, motion=motion, omm=omm):
            motion.update(omm, out=cpg.drive)
            sim.step_replay(cpg.advance(20), cpg.act_ids, 0, 20)

        runs.append((sim, cpg, motion, omm, tick))
    (s0, c0, m0, omm0, eager), (s1, c1, m1, omm1, captured) = runs
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                              # captured before these detectors have ever been updated
        captured()
    frames = _readings(721, ticks=7, n=n, seed=9)
    state = spec.new_state(n, 721)
    drives = []
    for k in range(7):
        new = torch.as_tensor(np.array(frames[k]), device=s0.device)
        omm0.copy_(new); omm1.copy_(new)
        g.replay()
        eager()
        torch.cuda.synchronize()
        want = spec.update(state, frames[k], m1.pairs, m1.weights, dt=DT, front=m1.front_edge, gain=40.0)
        assert torch.equal(c0.drive, c1.drive) and torch.equal(c0.phase, c1.phase) and torch.equal(c0.magnitude, c1.magnitude), k
        for name in FIELDS + ("fresh",):
            assert torch.equal(getattr(m0, name), getattr(m1, name)), (k, name)
        for key in keys:
            assert torch.equal(s0.field(key), s1.field(key)), (k, key)
        drives.append(c1.drive.clone())
    assert not torch.equal(drives[1], drives[-1]) and bool(torch.isfinite(s1.field("qpos")).all())
    _assert_equal_bits("the last replay", m1, c1.drive, state, want)
    m0.close(); m1.close(); c0.close(); c1.close()


def _yaw(q):
    w, x, y, z = q[:, 3], q[:, 4], q[:, 5], q[:, 6]
    return np.arctan2(2 * (w * z + x * y), 1 - 2 * (y * y + z * z))


def test_the_reflex_holds_the_course_on_a_checker_ground(torch_mod):
    """2 x 16 walking flies over a black-and-white checker of 2 mm squares: 500 ticks of ``render_into`` -> ``update`` ->
    ``cpg.step(20)``; the first group's drive comes from detectors with the default parameters, the second's from detectors with
    ``delta = 0`` (the reflex off).  Asserted: finite states, no contact overflow, drives inside [drive_min, drive_max], the second
    group's drive exactly ``base`` throughout, and the mean |yaw change| of the reflex group below the control group's.  The sizes
    are findings, printed here and recorded in profiles/motion_summary.md."""
    torch = torch_mod
    from flygym_amd.controllers import TurningCPG
    from flygym_amd.sensors import MotionDetectors
    from flygym_amd.vision import EyeRenderer, Scene

    n, steps = 32, 20
    sim, fly = _walking_batch(n, copy=3)
    dt = steps * float(sim.timestep)
    eyes = EyeRenderer(sim, fly.name, scene=Scene(checker_size=2.0, ground_rgb=((0, 0, 0), (1, 1, 1))))
    omm = torch.zeros((n, 2, 721, 2), dtype=torch.float32, device=sim.device)
    lo, hi = spec.DEFAULTS["drive_min"], spec.DEFAULTS["drive_max"]
    with TurningCPG(sim, fly.name) as cpg, MotionDetectors(sim, fly.name, dt=dt) as reflex, MotionDetectors(sim, fly.name, dt=dt, delta=0.0) as off:
        y0 = _yaw(sim.field("qpos").cpu().numpy().astype(np.float64))
        least = torch.full((n, 2), float("inf"), device=sim.device)
        most = torch.full((n, 2), float("-inf"), device=sim.device)
        control_at_base = torch.ones((), dtype=torch.bool, device=sim.device)
        for k in range(500):
            eyes.render_into(omm)
            reflex.update(omm)
            off.update(omm)
            cpg.drive[:16] = reflex.drive[:16]
            cpg.drive[16:] = off.drive[16:]
            least, most = torch.minimum(least, cpg.drive), torch.maximum(most, cpg.drive)
            control_at_base &= (off.drive == 1).all()
            cpg.step(steps)
        torch.cuda.synchronize()
        qpos, qvel = sim.field("qpos").cpu().numpy().astype(np.float64), sim.field("qvel").cpu().numpy()
        turn = np.degrees(np.angle(np.exp(1j * (_yaw(qpos) - y0)))).reshape(2, 16)
        for name, grp in zip(("reflex on", "reflex off"), turn):
            print(f"checker ground, {name}: yaw change mean {grp.mean():+.1f} deg, mean |yaw change| {np.abs(grp).mean():.1f}, "
                  f"spread (std) {grp.std():.1f}, min {grp.min():+.1f}, max {grp.max():+.1f}")
        print(f"drive range of the reflex group: {float(least[:16].min()):.3f} .. {float(most[:16].max()):.3f}; "
              f"last rotation signal mean {float(reflex.rotation[:16].mean()):+.3e}")
        assert np.isfinite(qpos).all() and np.isfinite(qvel).all() and bool(torch.isfinite(cpg.phase).all())
        assert bool(torch.isfinite(reflex.fast).all()) and bool(torch.isfinite(reflex.slow).all())
        assert sim.overflow_steps() == 0
        assert float(least.min()) >= f32(lo) and float(most.max()) <= f32(hi)
        assert bool(control_at_base)
        assert np.abs(turn[0]).mean() < np.abs(turn[1]).mean(), turn.mean(axis=1)


def test_refusals_come_before_anything_is_launched(torch_mod):
    torch = torch_mod
    from flygym_amd import _native
    from flygym_amd.sensors import MotionDetectors, Retina, _MotionParams

    sim, fly = _plain_batch()
    dev = sim.device
    motion = MotionDetectors(sim, fly.name, dt=DT)
    assert motion.front_edge == (1, 0) and motion.n_pairs == 2070
    omm = torch.zeros((N, 2, 721, 2), dtype=torch.float32, device=dev)
    out = torch.zeros((N, 2), dtype=torch.float32, device=dev)
    views = ("fast", "slow", "flow", "rotation", "translation", "drive")
    for name in views:
        getattr(motion, name).fill_(-5.0)
    motion.sums.fill_(-5)
    bad = [dict(omm=omm[:-1]), dict(omm=omm[:, :1]), dict(omm=torch.zeros((N, 2, 720, 2), device=dev)), dict(omm=omm.double()),
           dict(omm=omm.cpu()), dict(omm=torch.zeros((N, 2, 2, 721), device=dev).transpose(2, 3)), dict(omm=omm.cpu().numpy()),
           dict(omm=omm, base=out[:-1]), dict(omm=omm, base=out.double()), dict(omm=omm, base=out.cpu()), dict(omm=omm, base=1.0),
           dict(omm=omm, base=torch.zeros((2, N), device=dev).t()), dict(omm=omm, out=out[:-1]), dict(omm=omm, out=out.cpu()),
           dict(omm=omm, out=torch.zeros((2, N), device=dev).t()), dict(omm=omm, out=out.double())]
    for kw in bad:
        with pytest.raises(ValueError):
            motion.update(**kw)
    with pytest.raises(ValueError, match="shape"):
        motion.reset(np.zeros(N - 1, dtype=bool))
    ok_pairs = np.array([[0, 1]], dtype=np.int32), np.array([[1.0, 0.0]], dtype=f32)
    with pytest.raises(ValueError, match="1024"):
        MotionDetectors(sim, fly.name, dt=DT, retina=Retina(id_map=np.arange(1, 1026, dtype=np.int16).reshape(25, 41)), pairs=ok_pairs)
    many = np.stack([np.zeros(3073), 1 + np.arange(3073) % 720], axis=-1).astype(np.int32)
    with pytest.raises(ValueError, match="3072"):
        MotionDetectors(sim, fly.name, dt=DT, pairs=(many, np.ones((3073, 2), dtype=f32)))
    for wrong in ([[0, 721]], [[-1, 3]]):
        with pytest.raises(ValueError, match="outside the retina"):
            MotionDetectors(sim, fly.name, dt=DT, pairs=(np.array(wrong, dtype=np.int32), ok_pairs[1]))
    with pytest.raises(ValueError, match="a == b"):
        MotionDetectors(sim, fly.name, dt=DT, pairs=(np.array([[5, 5]], dtype=np.int32), ok_pairs[1]))
    with pytest.raises(ValueError):
        MotionDetectors(sim, fly.name, dt=DT, pairs=(np.array([[0.0, 1.0]]), ok_pairs[1]))               # (indices that are not integers)
    with pytest.raises(ValueError):
        MotionDetectors(sim, fly.name, dt=DT, pairs=(ok_pairs[0], np.ones((2, 2), dtype=f32)))
    with pytest.raises(ValueError, match="positive"):
        MotionDetectors(sim, fly.name, dt=0.0)
    with pytest.raises(ValueError):
        MotionDetectors(sim, "nosuchfly", dt=DT)
    # the cases the class cannot state, through the C ABI: a null handle or a status, with the reason
    lib = _native.lib()
    assert ctypes.sizeof(_MotionParams) == lib.nmf_motion_params_size() == 36
    p, stream = motion._params, sim._stream()
    pairs, weights = motion.pairs, motion.weights

    def create(params, pr, wt, n_pairs, n_omm):
        h = lib.nmf_motion_create(sim._batch_h, params, None if pr is None else pr.ctypes.data, None if wt is None else wt.ctypes.data, n_pairs, n_omm)
        if h:
            lib.nmf_motion_destroy(h)
        return h

    outside, itself = pairs.copy(), pairs.copy()
    outside[2069] = (3, 721)
    itself[7] = (9, 9)
    nan_weight = weights.copy()
    nan_weight[4, 1] = np.nan
    nan_gain = _MotionParams.from_buffer_copy(p)
    nan_gain.gain = float("nan")
    wide = _MotionParams.from_buffer_copy(p)
    wide.a_slow = 1.5
    for args, message in [((ctypes.byref(p), pairs, weights, 2070, 0), "n_omm must be in 1..1024"),
                          ((ctypes.byref(p), pairs, weights, 2070, 1025), "n_omm must be in 1..1024"),
                          ((ctypes.byref(p), pairs, weights, 3073, 721), "n_pairs must be in 0..3072"),
                          ((ctypes.byref(p), pairs, weights, -1, 721), "n_pairs must be in 0..3072"),
                          ((ctypes.byref(p), None, weights, 2070, 721), "null pairs / weights"),
                          ((ctypes.byref(p), outside, weights, 2070, 721), "pair 2069 = (3, 721) is outside the retina's 721"),
                          ((ctypes.byref(p), pairs, weights, 2070, 700), "is outside the retina's 700"),
                          ((ctypes.byref(p), itself, weights, 2070, 721), "pair 7 joins ommatidium 9 to itself (a == b)"),
                          ((ctypes.byref(p), pairs, nan_weight, 2070, 721), "the weight of pair 4 is not finite"),
                          ((ctypes.byref(nan_gain), pairs, weights, 2070, 721), "a parameter is not finite"),
                          ((ctypes.byref(wide), pairs, weights, 2070, 721), "a_fast and a_slow must be in [0, 1]"),
                          ((None, pairs, weights, 2070, 721), "null batch / params")]:
        assert not create(*args) and message in lib.nmf_last_error().decode(), message
    assert create(ctypes.byref(p), None, None, 0, 5)                                       # (no pairs: nothing to upload)
    h = motion._handle()
    for args, message in [((None, omm.data_ptr(), None, out.data_ptr()), "null handle"), ((h, None, None, out.data_ptr()), "null omm"),
                          ((h, omm.data_ptr(), None, None), "null drive"), ((h, omm.data_ptr() + 4, None, out.data_ptr()), "aligned"),
                          ((h, omm.data_ptr(), out.data_ptr() + 2, out.data_ptr()), "aligned")]:
        assert lib.nmf_motion_update(*args, stream) != 0 and message in lib.nmf_last_error().decode(), message
    assert lib.nmf_motion_reset(None, None, stream) != 0 and "null handle" in lib.nmf_last_error().decode()
    assert not lib.nmf_motion_field_ptr(h, 8, None) and "no such field" in lib.nmf_last_error().decode()
    torch.cuda.synchronize()
    for name in views:
        assert bool((getattr(motion, name) == -5).all()), name
    assert bool((motion.sums == -5).all()) and bool((out == 0).all()) and bool((motion.fresh == 1).all())
    omm[..., 0] = 0.5                                       # (a first update of constant readings: no flow, the base drive)
    assert motion.update(omm) is motion.drive
    torch.cuda.synchronize()
    assert bool((motion.drive == 1).all()) and bool((motion.flow == 0).all()) and bool((motion.fast == 0.5).all()) and bool((motion.fresh == 0).all())
    motion.close()
    assert motion.drive is None
    with pytest.raises(RuntimeError, match="closed"):
        motion.update(omm)


def test_a_multi_fly_world_resolves_to_the_flys_batch(torch_mod):
    torch = torch_mod
    from flygym_amd.sensors import MotionDetectors

    sim, fly = _plain_batch(4)

    class Several:                                         # what MotionDetectors asks of a MultiFlyHIPSimulation
        def for_fly(self, name):
            assert name == fly.name
            return sim

    frames = _readings(721, ticks=2, n=4, seed=2)
    with MotionDetectors(Several(), fly.name, dt=DT) as motion:
        assert motion.sim is sim
        state = spec.new_state(4, 721)
        for k in range(2):
            d = motion.update(torch.as_tensor(np.array(frames[k]), device=sim.device))
            torch.cuda.synchronize()
            want = spec.update(state, frames[k], motion.pairs, motion.weights, dt=DT, front=motion.front_edge)
        _assert_equal_bits("for_fly", motion, d, state, want)
