"""Sensory steering on the GPU (``flygym_amd/csrc/nmf_taxis.hip``, ``flygym_amd.controllers.SensorySteering``) against its numpy
specification ``tests/taxis_spec.py``.

Every comparison with the specification is bit for bit: the kernel's sums are integers, its quotients correctly rounded divisions
of exact operands and its float32 rule is compiled without contraction or reassociation."""
import ctypes
import functools

import numpy as np
import pytest

import taxis_spec as spec

pytestmark = pytest.mark.gpu

f32 = np.float32
N = 67                                       # prime: the last workgroup holds three worlds of four
# image sizes of the synthetic retinas: 2047 a side puts a centre at the end of the int16 range
SHAPES = {1: (5, 7), 63: (33, 61), 64: (64, 64), 65: (9, 2047), 1024: (2047, 40)}
GAINS = (1.5, -0.7, 0.25, -2.0, 0.0, 1.0, -0.125, 3.0)


@pytest.fixture
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch


def _bits(x):
    return np.ascontiguousarray(x, dtype=f32).view(np.int32)


@functools.lru_cache(maxsize=None)
def _plain_batch(n=N):
    """n worlds of the benchmark fly, never stepped: something for a SensorySteering to belong to."""
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
    """The default retina for 721 ommatidia; otherwise a synthetic one: up to three scattered pixels per ommatidium, the first
    ommatidium the first pixel alone, the last one the last pixel alone (its centre: the largest the table can hold)."""
    from flygym_amd.sensors import Retina

    if n_omm == 721:
        return Retina()
    H, W = SHAPES[n_omm]
    rng = np.random.default_rng(100 + n_omm)
    ids = np.zeros(H * W, dtype=np.int16)
    if n_omm == 1:
        ids[rng.choice(H * W, 3, replace=False)] = 1
    else:
        inner = rng.choice(np.arange(1, H * W - 1), min(H * W - 2, 3 * (n_omm - 2)), replace=False)
        ids[inner] = 2 + np.arange(inner.size) % max(n_omm - 2, 1) if n_omm > 2 else 0
        ids[0], ids[-1] = 1, n_omm
    return Retina(id_map=ids.reshape(H, W))


@functools.lru_cache(maxsize=None)
def _readings(n_omm, seed=0):
    """(N, 2, n_omm, 2) float32, read-only: world 0 all dark, 1 none dark, 2 one dark ommatidium (the last index, left eye; the
    first, right eye), 3 every reading exactly at the threshold (not dark), 4 at the threshold but one a unit in the last place
    below; the rest about 5 % dark.  A reading sits in one channel, the other is 0."""
    rng = np.random.default_rng(1000 * n_omm + seed)
    thr = f32(spec.DEFAULTS["obj_threshold"])
    r = rng.uniform(0.2, 1.0, (N, 2, n_omm)).astype(f32)
    dark = rng.random((N, 2, n_omm)) < 0.05
    r[dark] = rng.uniform(0.0, 0.1499, int(dark.sum())).astype(f32)
    r[0] = rng.uniform(0.0, 0.1, (2, n_omm)).astype(f32)
    r[1] = np.maximum(r[1], f32(0.2))
    r[2] = f32(0.6)
    r[2, 0, -1], r[2, 1, 0] = 0.0, 0.01
    r[3] = thr
    r[4] = thr
    r[4, 0, n_omm // 2] = np.nextafter(thr, f32(0))
    pale = rng.random(n_omm) < 0.3
    omm = np.zeros((N, 2, n_omm, 2), dtype=f32)
    omm[..., 0] = np.where(pale, 0, r)
    omm[..., 1] = np.where(pale, r, 0)
    omm.setflags(write=False)
    return omm


@functools.lru_cache(maxsize=None)
def _odor(n_dims, seed=0):
    """(N, n_dims, 4) float32, read-only: world 0 no odor anywhere (s_d = 0), 1 odor on the left sites only, 2 on the right
    only, 3 the same on both sides; the rest seeded, every fifth dimension-world pair without odor."""
    rng = np.random.default_rng(77 + 10 * n_dims + seed)
    odor = rng.uniform(0.0, 5.0, (N, n_dims, 4)).astype(f32)
    odor[rng.random((N, n_dims)) < 0.2] = 0.0
    odor[0] = 0.0
    odor[1:4] = rng.uniform(0.5, 5.0, (3, n_dims, 4)).astype(f32)
    odor[1][:, [1, 3]] = 0.0
    odor[2] = odor[1][:, [1, 0, 3, 2]]                                         # (world 1 mirrored)
    odor[3][:, 1], odor[3][:, 3] = odor[3][:, 0], odor[3][:, 2]
    odor.setflags(write=False)
    return odor


def _spec_update(steer, omm, odor, **params):
    r = steer.retina
    return spec.update(omm=omm, odor=odor, table=r.centre_table(), height=r.height, width=r.width, gains=steer.odor_gains,
                       front=steer.front_edge, n_worlds=steer.n_worlds, **params)


def _assert_equal_bits(label, steer, drive, want):
    for name, got, ref in zip(("features", "bias", "drive"), (steer.features, steer.bias, drive), want):
        got = got.cpu().numpy()
        same = _bits(got) == _bits(ref)
        assert same.all(), f"{label}: {name} differs in {int((~same).sum())} of {same.size} values, first at {np.argwhere(~same)[0].tolist()}"


@pytest.mark.parametrize("n_omm", [1, 63, 64, 65, 721, 1024])
def test_the_kernel_equals_the_specification_bit_for_bit(torch_mod, n_omm):
    torch = torch_mod
    from flygym_amd.controllers import SensorySteering

    sim, fly = _plain_batch()
    retina = _retina(n_omm)
    assert retina.num_ommatidia == n_omm
    if n_omm in (65, 1024):
        assert int(retina.centre_table().max()) == 16 * 2047 - 8             # the last pixel's centre, 2046.5 px
    omm_host = _readings(n_omm)
    omm = torch.as_tensor(np.array(omm_host), device=sim.device)
    seen = set()
    for n_dims in (0, 1, 8):
        steer = SensorySteering(sim, fly.name, retina=retina, odor_gains=GAINS[:n_dims], base=0.95)
        assert tuple(steer.features.shape) == (N, 2, 3) and tuple(steer.bias.shape) == (N,) and tuple(steer.drive.shape) == (N, 2)
        odor_host = _odor(n_dims)
        odor = torch.as_tensor(np.array(odor_host), device=sim.device)
        for label, a, b, ha, hb in (("omm", omm, None, omm_host, None), ("odor", None, odor, None, odor_host), ("both", omm, odor, omm_host, odor_host)):
            steer.features.fill_(-7.0); steer.bias.fill_(-7.0); steer.drive.fill_(-7.0)
            drive = steer.update(omm=a, odor=b)
            assert drive is steer.drive
            torch.cuda.synchronize()
            want = _spec_update(steer, ha, hb, base=0.95)
            _assert_equal_bits(f"n_omm {n_omm}, n_dims {n_dims}, {label}", steer, drive, want)
            seen.update(np.unique(want[2]).tolist())
        if n_dims == 8:                                     # the scenario is not trivial: what the special worlds promise
            feat, b, d = want
            assert feat[0, :, 2].tolist() == [1.0, 1.0] and feat[1].tolist() == [[0.5, 0.5, 0.0]] * 2
            assert feat[2, :, 2].tolist() == [f32(1 / n_omm)] * 2 and feat[3].tolist() == [[0.5, 0.5, 0.0]] * 2
            assert feat[4, 0, 2] == f32(1 / n_omm) and feat[4, 1, 2] == 0
            assert b[0] == 0 and b[3] == 0 and b[1] != 0 and b[2] == -b[1] and (b > 0).any() and (b < 0).any()
    assert len(seen) > 20                                                      # drives of many values, not a constant


def test_a_default_update_writes_into_the_callers_tensor(torch_mod):
    """``out=``: the drive lands in the caller's tensor (here a view into a larger one, as ``cpg.drive`` is a view of the
    controller's state) and ``.drive`` is left alone; default parameters."""
    torch = torch_mod
    from flygym_amd.controllers import SensorySteering

    sim, fly = _plain_batch()
    steer = SensorySteering(sim, fly.name, odor_gains=(1.0,))
    omm_host, odor_host = _readings(721, seed=3), _odor(1, seed=3)
    big = torch.full((N + 2, 2), -3.0, dtype=torch.float32, device=sim.device)
    steer.drive.fill_(-5.0)
    out = steer.update(omm=torch.as_tensor(np.array(omm_host), device=sim.device), odor=torch.as_tensor(np.array(odor_host), device=sim.device),
                       out=big[1:N + 1])
    torch.cuda.synchronize()
    _assert_equal_bits("out=", steer, out, _spec_update(steer, omm_host, odor_host))
    assert bool((big[0] == -3).all()) and bool((big[-1] == -3).all()) and bool((steer.drive == -5).all())


def _place_spheres(torch, sim, fly, azimuths_deg, distance=8.0, radius=2.0):
    """(n, 1, 4) float32 on the device: per world a sphere ``distance`` mm from the point between the eyes at the given azimuth
    from the fly's heading, at eye height; ``None``: far below the ground (no eye sees it)."""
    names = [s.name for s in fly.get_bodysegs_order()]
    eyes = sim.field("seg_xpos").reshape(sim.n_worlds, -1, 3)[:, [names.index("l_eye"), names.index("r_eye")]].mean(dim=1).cpu().numpy()
    q = sim.field("qpos").cpu().numpy().astype(np.float64)
    yaw = np.arctan2(2 * (q[:, 3] * q[:, 6] + q[:, 4] * q[:, 5]), 1 - 2 * (q[:, 5] ** 2 + q[:, 6] ** 2))
    out = np.zeros((sim.n_worlds, 1, 4), dtype=f32)
    for w, az in enumerate(azimuths_deg):
        if az is None:
            out[w, 0] = (0.0, 0.0, -100.0, radius)
        else:
            a = yaw[w] + np.deg2rad(az)
            out[w, 0] = (eyes[w, 0] + distance * np.cos(a), eyes[w, 1] + distance * np.sin(a), eyes[w, 2], radius)
    return torch.as_tensor(out, device=sim.device)


def test_real_readings_give_the_specifications_features(torch_mod):
    """Six worlds, a black sphere per world at +-30, +-70 and 150 degrees and none: the features of the rendered readings equal the
    specification applied to the same readings on the host; the eye on the sphere's side finds it.  Without a sphere in the
    scene every area is 0 and every drive 1, exactly."""
    torch = torch_mod
    from flygym_amd.controllers import SensorySteering
    from flygym_amd.vision import EyeRenderer, Scene

    azimuths = (30.0, -30.0, 70.0, -70.0, 150.0, None)
    sim, fly = _walking_batch(len(azimuths))
    steer = SensorySteering(sim, fly.name)
    eyes = EyeRenderer(sim, fly.name, scene=Scene(spheres=[(0, 0, -100, 2)], sphere_rgb=[(0, 0, 0)]))
    eyes.set_spheres(_place_spheres(torch, sim, fly, azimuths))
    omm = eyes.render()
    drive = steer.update(omm=omm)
    torch.cuda.synchronize()
    want = _spec_update(steer, omm.cpu().numpy(), None)
    _assert_equal_bits("rendered", steer, drive, want)
    feat, d = steer.features.cpu().numpy(), drive.cpu().numpy()
    print("rendered features (cy, cx, area) per world and eye:", feat.round(4).tolist(), "drive:", d.tolist())
    thr = spec.DEFAULTS["area_threshold"]
    assert feat[0, 0, 2] > thr and d[0, 0] < d[0, 1] and feat[1, 1, 2] > thr and d[1, 1] < d[1, 0]      # +-30 degrees: its side's eye
    assert (feat[5, :, 2] == 0).all() and (d[5] == 1).all()
    empty = EyeRenderer(sim, fly.name)
    drive = steer.update(omm=empty.render())
    torch.cuda.synchronize()
    assert bool((steer.features[:, :, 2] == 0).all()) and bool((drive == 1).all())


def test_one_control_tick_is_one_captured_graph(torch_mod):
    """``update(out=cpg.drive)`` + ``cpg.advance(20)`` + ``step_replay`` captured once on the batch's stream (a single chain) and
    replayed seven times with new readings written in place: every field of the batch and the controller's phase equal the eager
    run's."""
    torch = torch_mod
    from flygym_amd.controllers import SensorySteering, TurningCPG

    n = 16
    keys = ("qpos", "qvel", "ctrl", "qacc_warmstart", "seg_xpos", "seg_xquat", "site_xpos", "actuator_force", "sensordata", "time",
            "stats", "qacc", "stats_sum", "contact_geom", "act")
    runs = []
    for copy in (1, 2):
        sim, fly = _walking_batch(n, copy)
        cpg = TurningCPG(sim, fly.name)
        steer = SensorySteering(sim, fly.name, odor_gains=(1.0, -0.5))
        omm = torch.zeros((n, 2, 721, 2), dtype=torch.float32, device=sim.device)
        odor = torch.zeros((n, 2, 4), dtype=torch.float32, device=sim.device)

        def tick(sim=sim, cpg=cpg, steer=steer, omm=omm, odor=odor):
            steer.update(omm=omm, odor=odor, out=cpg.drive)
            sim.step_replay(cpg.advance(20), cpg.act_ids, 0, 20)

        runs.append((sim, cpg, steer, omm, odor, tick))
    (s0, c0, t0, omm0, odor0, eager), (s1, c1, t1, omm1, odor1, captured) = runs
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                              # captured before this steering object has ever been updated
        captured()
    drives = []
    for k in range(7):
        new_omm = torch.as_tensor(np.array(_readings(721, seed=10 + k)[:n]), device=s0.device)
        new_odor = torch.as_tensor(np.array(_odor(2, seed=10 + k)[:n]), device=s0.device)
        omm0.copy_(new_omm); omm1.copy_(new_omm); odor0.copy_(new_odor); odor1.copy_(new_odor)
        g.replay()
        eager()
        torch.cuda.synchronize()
        assert torch.equal(c0.drive, c1.drive) and torch.equal(c0.phase, c1.phase) and torch.equal(c0.magnitude, c1.magnitude), k
        assert torch.equal(t0.features, t1.features) and torch.equal(t0.bias, t1.bias), k
        for key in keys:
            assert torch.equal(s0.field(key), s1.field(key)), (k, key)
        drives.append(c1.drive.clone())
    assert not torch.equal(drives[0], drives[-1]) and bool(torch.isfinite(s1.field("qpos")).all())
    want = _spec_update(t1, np.array(_readings(721, seed=16)[:n]), np.array(_odor(2, seed=16)[:n]))
    _assert_equal_bits("the last replay", t1, c1.drive, want)
    c0.close(); c1.close()


def test_refusals_come_before_anything_is_launched(torch_mod):
    torch = torch_mod
    from flygym_amd import _native
    from flygym_amd.controllers import SensorySteering, _TaxisParams
    from flygym_amd.sensors import Retina

    sim, fly = _plain_batch()
    steer = SensorySteering(sim, fly.name, odor_gains=(1.0, 2.0))
    assert steer.front_edge == (1, 0)
    dev = sim.device
    omm = torch.zeros((N, 2, 721, 2), dtype=torch.float32, device=dev)
    odor = torch.zeros((N, 2, 4), dtype=torch.float32, device=dev)
    out = torch.zeros((N, 2), dtype=torch.float32, device=dev)
    steer.drive.fill_(-5.0); steer.features.fill_(-5.0); steer.bias.fill_(-5.0)
    bad = [dict(), dict(omm=omm[:-1]), dict(omm=omm[:, :1]), dict(omm=torch.zeros((N, 2, 720, 2), device=dev)), dict(omm=omm.double()),
           dict(omm=omm.cpu()), dict(omm=torch.zeros((N, 2, 2, 721), device=dev).transpose(2, 3)), dict(omm=omm.cpu().numpy()),
           dict(odor=odor[:, :1]), dict(odor=torch.zeros((N, 3, 4), device=dev)), dict(odor=odor.half()), dict(odor=odor.cpu()),
           dict(odor=torch.zeros((N, 4, 2), device=dev).transpose(1, 2)), dict(omm=omm, out=out[:-1]), dict(omm=omm, out=out.cpu()),
           dict(omm=omm, out=torch.zeros((2, N), device=dev).t()), dict(odor=odor, out=out.double())]
    for kw in bad:
        with pytest.raises(ValueError):
            steer.update(**kw)
    with pytest.raises(ValueError, match="3 dimensions for 2 odor_gains"):
        steer.update(odor=torch.zeros((N, 3, 4), device=dev))
    with pytest.raises(ValueError, match="1024"):
        SensorySteering(sim, fly.name, retina=Retina(id_map=np.arange(1, 1026, dtype=np.int16).reshape(25, 41)))
    with pytest.raises(ValueError, match="2047"):
        SensorySteering(sim, fly.name, retina=Retina(id_map=np.ones((2, 2048), dtype=np.int16)))
    with pytest.raises(ValueError, match="at most 8"):
        SensorySteering(sim, fly.name, odor_gains=[1.0] * 9)
    with pytest.raises(ValueError):
        SensorySteering(sim, "nosuchfly")
    # the cases the class cannot state, through the C ABI: a status, with the reason
    lib = _native.lib()
    p = steer._params
    assert ctypes.sizeof(_TaxisParams) == lib.nmf_taxis_params_size() == 52
    c, g, f, b, d = steer.centres.data_ptr(), steer._gains.data_ptr(), steer.features.data_ptr(), steer.bias.data_ptr(), steer.drive.data_ptr()
    stream = sim._stream()
    call = lambda *a: lib.nmf_taxis_update(*a, stream)
    cases = [((None, c, 721, 512, 450, omm.data_ptr(), None, g, 0, N, f, b, d), "null params"),
             ((ctypes.byref(p), c, 1025, 512, 450, omm.data_ptr(), None, g, 0, N, f, b, d), "n_omm must be in 1..1024"),
             ((ctypes.byref(p), c, 0, 512, 450, omm.data_ptr(), None, g, 0, N, f, b, d), "n_omm must be in 1..1024"),
             ((ctypes.byref(p), c, 721, 2048, 450, omm.data_ptr(), None, g, 0, N, f, b, d), "height, width <= 2047"),
             ((ctypes.byref(p), None, 721, 512, 450, omm.data_ptr(), None, g, 0, N, f, b, d), "null centres"),
             ((ctypes.byref(p), c, 721, 512, 450, omm.data_ptr() + 4, None, g, 0, N, f, b, d), "aligned"),
             ((ctypes.byref(p), c, 721, 512, 450, None, odor.data_ptr(), g, 9, N, f, b, d), "n_dims must be in 0..8"),
             ((ctypes.byref(p), c, 721, 512, 450, None, odor.data_ptr(), g, -1, N, f, b, d), "n_dims must be in 0..8"),
             ((ctypes.byref(p), c, 721, 512, 450, None, odor.data_ptr(), None, 2, N, f, b, d), "null odor gains"),
             ((ctypes.byref(p), c, 721, 512, 450, None, None, g, 2, N, f, b, d), "both null"),
             ((ctypes.byref(p), c, 721, 512, 450, omm.data_ptr(), odor.data_ptr(), g, 2, N, f, b, None), "null drive"),
             ((ctypes.byref(p), c, 721, 512, 450, omm.data_ptr(), odor.data_ptr(), g, 2, 0, f, b, d), "n_worlds must be at least 1")]
    for args, message in cases:
        assert call(*args) != 0 and message in lib.nmf_last_error().decode(), message
    torch.cuda.synchronize()
    assert bool((steer.drive == -5).all()) and bool((steer.features == -5).all()) and bool((steer.bias == -5).all())
    omm.fill_(0.5)                                         # (nothing dark, no odor: the unit drive)
    assert call(ctypes.byref(p), c, 721, 512, 450, omm.data_ptr(), odor.data_ptr(), g, 2, N, None, None, d) == 0      # (outputs but the drive are optional)
    torch.cuda.synchronize()
    assert bool((steer.drive == 1).all()) and bool((steer.features == -5).all())


def test_a_multi_fly_world_resolves_to_the_flys_batch(torch_mod):
    torch = torch_mod
    from flygym_amd.controllers import SensorySteering

    sim, fly = _plain_batch(4)

    class Several:                                         # what SensorySteering asks of a MultiFlyHIPSimulation
        def for_fly(self, name):
            assert name == fly.name
            return sim

    steer = SensorySteering(Several(), fly.name, odor_gains=(1.0,))
    assert steer.sim is sim
    odor = torch.as_tensor(np.array(_odor(1)[:4]), device=sim.device)
    d = steer.update(odor=odor)
    torch.cuda.synchronize()
    _assert_equal_bits("for_fly", steer, d, _spec_update(steer, None, np.array(_odor(1)[:4])))


def _yaw(q):
    w, x, y, z = q[:, 3], q[:, 4], q[:, 5], q[:, 6]
    return np.arctan2(2 * (w * z + x * y), 1 - 2 * (y * y + z * z))


def test_a_sphere_steers_the_flies_towards_it(torch_mod):
    """3 x 16 worlds: a black sphere of radius 2 mm fixed 8 mm from the start pose at +40 degrees (left), at -40 degrees, and none;
    250 ticks of ``render_into`` -> ``update(out=cpg.drive)`` -> ``cpg.step(20)``.  Asserted: finite states, no contact overflow,
    every drive inside [drive_min, drive_max], the control group's drive exactly (1, 1) throughout, the first tick's drive lower on
    the sphere's side, and the +40 group's mean yaw change above the -40 group's.  Absolute headings are a finding (the open-loop
    gait itself curves): the three group means and spreads are printed.  Measured: +8.5 +- 0.9, -40.6 +- 0.4,
    -35.0 +- 3.3 degrees; the first tick's drives (0.4, 1), (1, 0.4), (1, 1)."""
    torch = torch_mod
    from flygym_amd.controllers import SensorySteering, TurningCPG
    from flygym_amd.vision import EyeRenderer, Scene

    n = 48
    sim, fly = _walking_batch(n, copy=3)
    steer = SensorySteering(sim, fly.name)
    eyes = EyeRenderer(sim, fly.name, scene=Scene(spheres=[(0, 0, -100, 2)], sphere_rgb=[(0, 0, 0)]))
    eyes.set_spheres(_place_spheres(torch, sim, fly, [40.0] * 16 + [-40.0] * 16 + [None] * 16))
    omm = torch.zeros((n, 2, 721, 2), dtype=torch.float32, device=sim.device)
    lo, hi = spec.DEFAULTS["drive_min"], spec.DEFAULTS["drive_max"]
    with TurningCPG(sim, fly.name) as cpg:
        y0 = _yaw(sim.field("qpos").cpu().numpy().astype(np.float64))
        least = torch.full((n, 2), float("inf"), device=sim.device)
        most = torch.full((n, 2), float("-inf"), device=sim.device)
        control_at_one = torch.ones((), dtype=torch.bool, device=sim.device)
        first = None
        for k in range(250):
            eyes.render_into(omm)
            steer.update(omm=omm, out=cpg.drive)
            if k == 0:
                first = cpg.drive.clone()
            least, most = torch.minimum(least, cpg.drive), torch.maximum(most, cpg.drive)
            control_at_one &= (cpg.drive[32:] == 1).all()
            cpg.step(20)
        torch.cuda.synchronize()
        qpos, qvel = sim.field("qpos").cpu().numpy().astype(np.float64), sim.field("qvel").cpu().numpy()
        turn = np.degrees(np.angle(np.exp(1j * (_yaw(qpos) - y0)))).reshape(3, 16)
        for name, grp in zip(("+40 deg", "-40 deg", "none"), turn):
            print(f"sensory steering, sphere at {name}: yaw change mean {grp.mean():+.1f} deg, spread (std) {grp.std():.1f}, "
                  f"min {grp.min():+.1f}, max {grp.max():+.1f}")
        first = first.cpu().numpy()
        print("first tick's drive (left, right): +40", first[0].tolist(), "-40", first[16].tolist(), "none", first[32].tolist())
        assert np.isfinite(qpos).all() and np.isfinite(qvel).all() and bool(torch.isfinite(cpg.phase).all())
        assert sim.overflow_steps() == 0
        assert float(least.min()) >= f32(lo) and float(most.max()) <= f32(hi)
        assert bool(control_at_one)
        assert (first[:16, 0] < first[:16, 1]).all() and (first[16:32, 1] < first[16:32, 0]).all()
        means = turn.mean(axis=1)
        assert means[0] > means[1], means
