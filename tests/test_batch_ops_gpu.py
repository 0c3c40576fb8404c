"""``nmf_gather_kernel``, ``nmf_scatter_kernel``, ``nmf_pack_obs_kernel`` (csrc/nmf_batch_ops.hip) and ``nmf_odor_kernel``
(csrc/nmf_sensors.hip) past one trip of their loops and one block of threads.

The gather / scatter launches cap the grid at 4096 blocks of 256 threads, the pack launch at 8192, and go on in a grid-stride
loop.  7800 worlds of the benchmark model is the smallest round count at which ``pack_observations`` (270 floats a world) has
more elements than 8192 x 256; ``get_body_rotations`` (69 x 4 a world) is then past 4096 x 256 as well.  Copies are compared
bit for bit with torch indexing of the fields, at 7800 worlds (built once for the module) and at 3 (less than one block).
The odor kernel (one thread per world and sensor) runs 67 worlds — 268 threads, a second block partly idle — with no source
and with a source a micrometre from a sensor, against ``sensors_oracle.odor_intensity`` in float64."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
BIG = 7800


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch


def _live_sim(torch, world, n_worlds, seed):
    """A batch whose worlds all differ — each fly somewhere else over the flat ground, with joint angles and velocities of its
    own — stepped once so that every field is live."""
    from flygym_amd import HIPSimulation

    sim = HIPSimulation(world, n_worlds=n_worlds, device=0)
    rng = np.random.default_rng(seed)
    offset = np.concatenate([rng.uniform(-5, 5, (n_worlds, 2)), rng.uniform(0, 0.5, (n_worlds, 1))], axis=1)
    qpos = sim.field("qpos")
    qpos[:, :3] += torch.as_tensor(offset, dtype=torch.float32, device=sim.device)
    qpos[:, 7:] += torch.as_tensor(rng.normal(0, 0.05, (n_worlds, qpos.shape[1] - 7)), dtype=torch.float32, device=sim.device)
    qvel = sim.field("qvel")
    v = rng.normal(0, 5, tuple(qvel.shape))
    v[:, :6] = rng.normal(0, 30, (n_worlds, 6))
    qvel[:] = torch.as_tensor(v, dtype=torch.float32, device=sim.device)
    sim.step(1)
    torch.cuda.synchronize()
    return sim


@pytest.fixture(scope="module")
def big(torch_mod):
    """(fly, sim) of 7800 worlds — a world of its own (``HIPSimulation`` rewrites the world it is given)."""
    from flygym_amd.models import make_model

    fly, world, _ = make_model()
    return fly, _live_sim(torch_mod, world, BIG, 1)


def _bits(t):
    import torch

    return t.contiguous().view(torch.int32)


def _check_gather(torch, sim, rng):
    n = sim.n_worlds
    cases = []
    for field, group in (("qpos", 1), ("seg_xpos", 3), ("seg_xquat", 4), ("site_xpos", 3)):
        width = sim.field(field).shape[1]
        assert width % group == 0 and (width > 0 or field == "site_xpos")      # (the benchmark model may have no sites)
        m = width // group
        if m == 0:
            continue
        cases += [(field, group, np.arange(m - 1, -1, -1)), (field, group, rng.integers(0, m, 2 * m + 7)),
                  (field, group, np.array([int(rng.integers(0, m))])), (field, group, rng.permutation(m))]
    for field, group, ids in cases:
        src = sim.field(field)
        assert torch.isfinite(src).all() and float(src.abs().max()) > 0
        got = sim._gather(field, sim._ids(ids), group)
        idx = torch.as_tensor(ids, dtype=torch.int64, device=sim.device)
        want = src[:, idx] if group == 1 else src.view(n, -1, group)[:, idx, :]
        assert tuple(got.shape) == ((n, len(ids)) if group == 1 else (n, len(ids), group))
        assert torch.equal(_bits(got), _bits(want)), f"{field} group {group}, {len(ids)} ids"
    return max(n * len(ids) * group for _, group, ids in cases)


def _check_getters(torch, sim, fly):
    n = sim.n_worlds
    assert torch.equal(_bits(sim.get_body_rotations(fly.name)), _bits(sim.field("seg_xquat").view(n, -1, 4)))
    assert torch.equal(_bits(sim.get_body_positions(fly.name)), _bits(sim.field("seg_xpos").view(n, -1, 3)))
    assert torch.equal(_bits(sim.get_site_positions(fly.name)), _bits(sim.field("site_xpos").view(n, sim.model.nsite, 3)))
    nj = sim.model.nv - 6
    assert torch.equal(_bits(sim.get_joint_angles(fly.name)), _bits(sim.field("qpos")[:, 7:7 + nj]))
    assert torch.equal(_bits(sim.get_joint_velocities(fly.name)), _bits(sim.field("qvel")[:, 6:6 + nj]))


def _check_scatter(torch, sim, fly):
    from flygym_amd.compose import ActuatorType

    n = sim.n_worlds
    ctrl = sim.field("ctrl")
    before = ctrl.clone()
    ids = sim.replay_ids(fly.name).to(torch.int64)
    assert ids.numel() == 42 and ctrl.shape[1] > 42                     # the adhesion columns stay untouched
    vals = (torch.arange(n * 42, dtype=torch.float32, device=sim.device) + 0.5).view(n, 42)    # exact: < 2^24
    try:
        sim.set_actuator_inputs(fly.name, ActuatorType.POSITION, vals)
        want = before.clone()
        want[:, ids] = vals
        assert torch.equal(_bits(ctrl), _bits(want))
        assert not torch.equal(ctrl, before)
    finally:
        ctrl.copy_(before)


def _check_pack(torch, sim):
    n, nj = sim.n_worlds, sim.model.nv - 6
    assert 2 * nj + 42 + 96 == 270
    out = torch.full((n, 300), -12345.0, dtype=torch.float32, device=sim.device)
    sim.pack_observations(out)
    want = torch.cat([sim.field("qpos")[:, 7:7 + nj], sim.field("qvel")[:, 6:6 + nj], sim.field("actuator_force")[:, :42],
                      sim.field("sensordata"), torch.full((n, 30), -12345.0, dtype=torch.float32, device=sim.device)], dim=1)
    assert torch.equal(_bits(out), _bits(want))
    for lo, hi in ((0, nj), (nj, 2 * nj), (2 * nj, 2 * nj + 42)):       # (the contact block may be all 0: a fly in the air)
        assert float(want[:, lo:hi].abs().max()) > 0 and not torch.equal(want[0, lo:hi], want[n - 1, lo:hi])


def test_gather_past_the_grid_cap(torch_mod, big):
    fly, sim = big
    most = _check_gather(torch_mod, sim, np.random.default_rng(21))
    assert most > 4096 * 256 and BIG * 69 * 4 > 4096 * 256
    _check_getters(torch_mod, sim, fly)


def test_scatter_of_the_actuator_inputs_at_7800_worlds(torch_mod, big):
    fly, sim = big
    _check_scatter(torch_mod, sim, fly)


def test_scatter_past_the_grid_cap(torch_mod, big):
    """``set_actuator_inputs`` writes 42 columns: 7800 worlds stay within 4096 x 256 elements.  140 ids — a permutation of the
    control columns three times over, each column given the same value every time, so the order of the writes cannot show —
    take the scatter kernel's loop into its second trip."""
    torch = torch_mod
    from flygym_amd import _native

    fly, sim = big
    ctrl = sim.field("ctrl")
    nu = ctrl.shape[1]
    rng = np.random.default_rng(22)
    ids = np.concatenate([rng.permutation(nu) for _ in range(-(-140 // nu))])[:140]
    assert BIG * len(ids) > 4096 * 256 and len(set(ids.tolist())) == nu
    col_vals = (torch.arange(BIG * nu, dtype=torch.float32, device=sim.device) + 0.25).view(BIG, nu)
    idx = torch.as_tensor(ids, dtype=torch.int64, device=sim.device)
    src = col_vals[:, idx].contiguous()
    before = ctrl.clone()
    try:
        _native.check(_native.lib().nmf_scatter(sim._batch_h, _native.FIELDS["ctrl"], sim._ids(ids).data_ptr(), len(ids),
                                                src.data_ptr(), sim._stream()))
        assert torch.equal(_bits(ctrl), _bits(col_vals))
    finally:
        ctrl.copy_(before)


def test_pack_observations_past_the_grid_cap(torch_mod, big):
    _, sim = big
    assert BIG * 270 > 8192 * 256 >= (BIG - 100) * 270
    _check_pack(torch_mod, sim)


def test_the_same_copies_within_one_block(torch_mod, bench_model):
    fly, world, _ = bench_model
    sim = _live_sim(torch_mod, world, 3, 2)
    assert _check_gather(torch_mod, sim, np.random.default_rng(23)) > 256 > 3 * 42
    _check_getters(torch_mod, sim, fly)
    _check_scatter(torch_mod, sim, fly)
    _check_pack(torch_mod, sim)


def _sensor_sites(sim, fly):
    """(segment indices, float32 offsets, float64 world positions (n_worlds, 4, 3) by the specification's formula)."""
    import sensors_oracle as so
    from flygym_amd.sensors import ODOR_SENSOR_SITES

    names = [s.name for s in fly.get_bodysegs_order()]
    seg = [names.index(n) for n, _ in ODOR_SENSOR_SITES]
    rel = np.array([r for _, r in ODOR_SENSOR_SITES], dtype=np.float32).astype(np.float64)
    n = sim.n_worlds
    xpos = sim.field("seg_xpos").cpu().numpy().reshape(n, -1, 3).astype(np.float64)
    xquat = sim.field("seg_xquat").cpu().numpy().reshape(n, -1, 4).astype(np.float64)
    pos = np.array([[xpos[w, sg] + so.quat_to_mat(xquat[w, sg]) @ rel[k] for k, sg in enumerate(seg)] for w in range(n)])
    return seg, rel, xpos, xquat, pos


def test_odor_kernel_partial_block_no_source_and_near_source(torch_mod, bench_model):
    torch = torch_mod
    import sensors_oracle as so
    from flygym_amd import _native
    from flygym_amd.sensors import OdorSensors

    fly, world, _ = bench_model
    n = 67                                                            # 268 threads: one full block and 12 of the next
    sim = _live_sim(torch, world, n, 3)
    seg, rel, xpos, xquat, pos = _sensor_sites(sim, fly)
    # ---- no source: every reading 0 (the Python class cannot state an empty odor field: the ABI call itself)
    seg_d = torch.as_tensor(np.array(seg, dtype=np.int32), device=sim.device)
    rel_d = torch.as_tensor(rel.astype(np.float32), device=sim.device)
    out = torch.full((n, 2, 4), -7.0, dtype=torch.float32, device=sim.device)
    _native.check(_native.lib().nmf_odor_intensity(sim._batch_h, seg_d.data_ptr(), rel_d.data_ptr(), 4, None, None, 0, 2,
                                                   out.data_ptr(), sim._stream()))
    assert tuple(out.shape) == (n, 2, 4) and bool((out == 0).all())
    # ---- three far sources and one 1e-3 mm from sensor 2 of world 40
    rng = np.random.default_rng(31)
    w_near, k_near = 40, 2
    far = rng.uniform(-20, 20, (3, 3)); far[:, 2] = rng.uniform(0.5, 3, 3)
    direction = np.array([2.0, -1.0, 2.0]) / 3.0
    src = np.concatenate([far, (pos[w_near, k_near] + 1e-3 * direction)[None]]).astype(np.float32)
    peak = rng.uniform(0.1, 1.0, (4, 2)).astype(np.float32)
    odor = OdorSensors(sim, fly.name, src, peak)
    got = odor.get_odor_intensities().cpu().numpy().astype(np.float64)
    src64, peak64 = src.astype(np.float64), peak.astype(np.float64)           # the reference reads the same inputs
    want = so.odor_intensity(xpos, xquat, seg, rel, src64, peak64)
    assert got.shape == want.shape == (n, 2, 4)
    ordinary = np.ones((n, 2, 4), dtype=bool)
    ordinary[w_near] = False                   # the other sensors of that world are within a millimetre of the source too
    gap = np.linalg.norm(np.delete(pos, w_near, axis=0) - src64[3], axis=-1).min()
    assert gap > 0.1, gap                      # the other worlds' flies stand elsewhere: ordinary readings
    np.testing.assert_allclose(got[ordinary], want[ordinary], rtol=2e-5)      # float32 vs float64: the existing test's bar
    # The near reading is peak / d^2 with d ~ 1e-3 between two points of magnitude |p|.  With u = 2^-24 (float32 unit
    # roundoff) the kernel's sensor position p = xpos + R(quat) rel carries, per component: u |p_i| from the final sum; from
    # R rel at most 7 u |rel|_1 — an entry of R is 1 - 2 (a + b) or 2 (a +- b) of products of quaternion components, at most 4 u
    # off, and the three-term dot product adds 3 u of its terms.  That is about one float32 ulp (2 u |p|) of the position's
    # magnitude per component, as a vector at most sqrt(3) times the largest component's bound.  The difference p - source is
    # exact (the two agree to within a factor of two in every component that matters, Sterbenz), so d^2 = |e|^2 is off by at
    # most 2 d |dp| + |dp|^2: the position error, divided by the distance, enters the reading twice.  The rest (the squares, the
    # sum, the division, the far sources) is the ordinary 2e-5.
    u = 2.0 ** -24
    d = np.linalg.norm(pos[w_near, k_near] - src64[3])
    assert 0.5e-3 < d < 2e-3
    dps = [np.sqrt(3.0) * u * (np.abs(pos[w_near, k]).max() + 7.0 * np.abs(rel[k]).sum()) for k in range(4)]
    dp = dps[k_near]
    bar = 2.0 * dp / d + (dp / d) ** 2 + 2e-5
    err = np.abs(got[w_near, :, k_near] / want[w_near, :, k_near] - 1.0).max()
    print(f"near source: d = {d:.4e} mm, position bound {dp:.3e} mm, bar {bar:.3e}, measured {err:.3e}")
    assert bar < 5e-3                                                          # (a bar that still means something)
    assert err <= bar
    assert want[w_near, :, k_near].min() > 1e4                                 # the near source dominates that reading
    # that world's other sensors: a fraction of a millimetre from the source, the same bound with their own distance
    for k in range(4):
        dk = np.linalg.norm(pos[w_near, k] - src64[3])
        np.testing.assert_allclose(got[w_near, :, k], want[w_near, :, k], rtol=2.0 * dps[k] / dk + (dps[k] / dk) ** 2 + 2e-5)
