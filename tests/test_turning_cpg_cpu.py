"""The closed-loop tripod CPG's specification (``tests/cpg_spec.py``) on the CPU: what it computes, and its C ABI.  The kernel is
tested against it in ``tests/test_turning_cpg_gpu.py``."""
import ctypes

import numpy as np
import pytest

import cpg_spec as spec

from flygym_amd.controllers import TripodCPG

DT = 1e-4


@pytest.fixture(scope="module")
def tripod():
    from flygym_amd.models import make_model

    fly = make_model()[0]
    return TripodCPG(fly.get_actuated_jointdofs_order("position"), DT)


def _unit(n):
    return np.ones((n, 6)), np.ones((n, 2))


def test_unit_drive_reproduces_the_tripod_table(tripod):
    """The tripod is a fixed point of the coupling: the float64 specification with the unit drive, reset to the world offsets
    w / n, equals ``TripodCPG.targets(3, 2500)`` within 1e-6 rad — three float32 roundings (the cycle's interpolation weights, the
    row, the table) of values below 4 rad; measured 2.4e-7.  Shards placed with first_world / total_worlds equal their rows."""
    r, d = _unit(3)
    rows, phases, mags, _, _ = spec.rollout(tripod.cycle, tripod.leg_of_dof, spec.reset_phases(3), r, d, 2500, timestep=DT)
    ref = tripod.targets(3, 2500)
    err = np.abs(rows - ref).max()
    print(f"float64 specification, unit drive, against TripodCPG.targets(3, 2500): {err:.3e} rad")
    assert err < 1e-6
    assert np.abs(ref).max() < 4.0
    assert np.array_equal(mags, np.ones_like(mags))
    # float32 flavour at r = 1: the row is the interpolated cycle itself
    rows32 = spec.rollout(tripod.cycle, tripod.leg_of_dof, spec.reset_phases(3), r, d, 300, timestep=DT, dtype=np.float32)[0]
    assert rows32.dtype == np.float32 and np.abs(rows32 - ref[:, :300]).max() < 1e-6
    r2, d2 = _unit(2)
    shard = spec.rollout(tripod.cycle, tripod.leg_of_dof, spec.reset_phases(2, first_world=4, total_worlds=8), r2, d2, 100, timestep=DT)[0]
    r8, d8 = _unit(8)
    whole = spec.rollout(tripod.cycle, tripod.leg_of_dof, spec.reset_phases(8), r8, d8, 100, timestep=DT)[0]
    np.testing.assert_array_equal(shard, whole[4:6])
    assert np.abs(shard - tripod.targets(2, 100, first_world=4, total_worlds=8)).max() < 1e-6


def test_perturbed_phases_lock_back_onto_the_tripod(tripod):
    """From phases perturbed by (0.1, -0.2, 0.05, 0.3, -0.1, 0.15) cycles the relative phases are within 5e-3 cycles of the
    tripod after 1000 steps and within 1e-6 after 2500 (measured 1.3e-3 and 1.6e-7)."""
    start = np.mod(spec.reset_phases(1) + np.array([[0.1, -0.2, 0.05, 0.3, -0.1, 0.15]]), 1.0)
    r, d = _unit(1)
    _, phases, _, end, _ = spec.rollout(tripod.cycle, tripod.leg_of_dof, start, r, d, 2500, timestep=DT)
    bias = spec.BIAS / (2 * np.pi)

    def lock_error(th):
        return float(np.abs(spec.wrap(th - th[0] - (bias - bias[0]))).max())

    e0, e1000, e2500 = lock_error(phases[0, 0]), lock_error(phases[0, 1000]), lock_error(end[0])
    print(f"phase-lock error (cycles) at step 0 / 1000 / 2500: {e0:.3e} / {e1000:.3e} / {e2500:.3e}")
    assert e0 > 0.2 and e1000 < 5e-3 and e2500 < 1e-6


def test_magnitudes_and_side_frequencies(tripod):
    """Magnitudes follow the closed form of their Euler recurrence, r_k = R + (1 - R)(1 - a dt)^k; a zero drive holds that
    side's phases, a negative drive runs them backwards at the same rate."""
    a, n = 20.0, 300
    drive = np.array([[0.4, 1.5], [0.0, 1.0], [-1.0, 1.0], [1.0, -0.7]])
    r0 = np.ones((4, 6))
    _, phases, mags, end, r_end = spec.rollout(tripod.cycle, tripod.leg_of_dof, spec.reset_phases(4), r0, drive, n, timestep=DT,
                                               convergence=a)
    R = np.abs(drive.astype(np.float32).astype(np.float64))[:, spec.SIDE]          # (the drive is a float32 input)
    k = np.arange(n)[None, :, None]
    np.testing.assert_allclose(mags, R[:, None, :] + (1 - R[:, None, :]) * (1 - a * DT) ** k, rtol=0, atol=1e-12)
    np.testing.assert_allclose(r_end, R + (1 - R) * (1 - a * DT) ** n, rtol=0, atol=1e-12)
    # sign(d) sets the direction a side's phases run in; seen exactly with the coupling off (with it on, the other side pulls)
    _, ph, _, _, _ = spec.rollout(tripod.cycle, tripod.leg_of_dof, spec.reset_phases(3), np.ones((3, 6)),
                                  np.array([[0.0, 1.0], [-1.0, 1.0], [1.0, 1.0]]), n, timestep=DT, coupling=0.0)
    moved = spec.wrap(ph[:, -1] - ph[:, 0])
    step = 12.0 * DT * (n - 1)
    np.testing.assert_allclose(moved[0, :3], 0.0, atol=1e-15)               # zero drive: held
    np.testing.assert_allclose(moved[0, 3:], step, atol=1e-12)
    np.testing.assert_allclose(moved[1, :3], -step, atol=1e-12)             # negative drive: backwards
    np.testing.assert_allclose(moved[2], step, atol=1e-12)
    # coupled network: a zero drive on both sides holds the tripod where it is, a negative one runs the whole gait backwards
    _, ph, _, _, _ = spec.rollout(tripod.cycle, tripod.leg_of_dof, spec.reset_phases(2), np.ones((2, 6)),
                                  np.array([[0.0, 0.0], [-1.0, -1.0]]), n, timestep=DT)
    moved = spec.wrap(ph[:, -1] - ph[:, 0])
    np.testing.assert_allclose(moved[0], 0.0, atol=1e-12)
    np.testing.assert_allclose(moved[1], -step, atol=1e-9)
    assert np.isfinite(phases).all() and np.isfinite(end).all()


def test_abi_of_the_controller():
    from flygym_amd import _native
    from flygym_amd.controllers import _CpgParams, TurningCPG, __all__ as exported

    _native.build()
    lib = _native.lib()
    assert ctypes.sizeof(_CpgParams) == lib.nmf_cpg_params_size()
    for name in ("nmf_cpg_params_size", "nmf_cpg_create", "nmf_cpg_destroy", "nmf_cpg_reset", "nmf_cpg_field_ptr", "nmf_cpg_advance"):
        assert hasattr(lib, name) and name in _native.exported_symbols(), name
    assert "TurningCPG" in exported and "TripodCPG" in exported and issubclass(TurningCPG, TripodCPG)
    # refusals that need no device
    assert lib.nmf_cpg_advance(None, 1, None, 1, None) != 0 and b"null controller" in lib.nmf_last_error()
    assert lib.nmf_cpg_reset(None, None, 0, 1, None) != 0
    assert not lib.nmf_cpg_create(None, None, None, None, None) and b"null batch" in lib.nmf_last_error()
    assert not lib.nmf_cpg_field_ptr(None, 0, None)
    lib.nmf_cpg_destroy(None)


def _yaw(q):
    w, x, y, z = q[3:7]
    return np.arctan2(2 * (w * z + x * y), 1 - 2 * (y * y + z * z))


def test_the_drive_steers_the_fly_on_the_oracle(tripod, bench_blob, oracle_lib):
    """One world, phase offset 0, 500-step settle, then 10 000 steps of the float64 specification's table on the float64 oracle
    under drives (1, 0.4), (1, 1), (0.4, 1): the state stays finite and the yaw change is ordered — the fly turns towards the
    weaker side.  Measured: -83.7, -65.9, +17.6 degrees (the open-loop gait curves by itself)."""
    _, m = bench_blob
    yaws = []
    for drive in ((1.0, 0.4), (1.0, 1.0), (0.4, 1.0)):
        rows, phases, mags, _, _ = spec.rollout(tripod.cycle, tripod.leg_of_dof, spec.reset_phases(1), np.ones((1, 6)),
                                                np.array([drive]), 10000, timestep=DT)
        assert np.isfinite(rows).all() and np.isfinite(phases).all() and np.isfinite(mags).all()
        o = oracle_lib.Oracle(m.to_blob(), "f64")
        o.ctrl[42:] = 1.0
        o.step(500)
        y0 = _yaw(o.qpos)
        o.step_replay(np.ascontiguousarray(rows[0], dtype=np.float32), np.arange(42), 0, 10000)
        assert np.isfinite(o.qpos).all()
        yaws.append(float(np.degrees(_yaw(o.qpos) - y0)))
    print("yaw change (deg) under drives (1, 0.4), (1, 1), (0.4, 1):", [round(y, 2) for y in yaws])
    assert yaws[0] < yaws[1] < yaws[2]
