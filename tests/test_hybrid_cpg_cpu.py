"""The hybrid turning controller's specification (``tests/hybrid_spec.py``) on the CPU: what the two rules compute, the lifting
property of the default correction vectors, and the C ABI.  The kernel is tested against it in ``tests/test_hybrid_cpg_gpu.py``."""
import ctypes
import re

import numpy as np
import pytest

import cpg_spec
import hybrid_spec as spec

from flygym_amd.controllers import TripodCPG

DT = 1e-4
NSEG, ROOT, TIPS = 9, 1, np.array([2, 3, 4, 5, 6, 8])          # a small segment list: root at 1, tips scattered
THR_H, THR_F = 0.05, 1.0


@pytest.fixture(scope="module")
def tripod():
    from flygym_amd.models import make_model

    fly, world, _ = make_model()
    cpg = TripodCPG(fly.get_actuated_jointdofs_order("position"), DT)
    model = world.compile_model()
    return cpg, fly, model, cpg.stance_bins(model, fly)


def _inputs(n, h=None, force=None, found=None, quat=(1.0, 0.0, 0.0, 0.0)):
    """seg_xpos (n, NSEG, 3), seg_xquat (n, NSEG, 4), sensordata (n, 96) with the legs ``h`` below a root at z = 1 and the world
    force ``force`` (n, 6, 3) on each leg."""
    xpos = np.zeros((n, NSEG, 3), dtype=np.float32)
    xpos[:, ROOT, 2] = 1.0
    xpos[:, TIPS, 2] = 1.0 - (np.full((n, 6), 0.5) if h is None else np.asarray(h))
    xquat = np.zeros((n, NSEG, 4), dtype=np.float32)
    xquat[:, :, 0] = 1.0
    xquat[:, ROOT] = quat
    sd = np.zeros((n, 6, 16), dtype=np.float32)
    if force is not None:
        sd[..., 1:4] = force
        sd[..., 0] = 1.0 if found is None else found
    sd[..., 10:13] = (0, 0, 1)
    sd[..., 13:16] = (0, 1, 0)
    return xpos, xquat, sd.reshape(n, 96)


def _decide(xpos, xquat, sd, phase, swing, **kw):
    kw = dict(dict(retraction_threshold=THR_H, stumbling_force_threshold=THR_F), **kw)
    return spec.decide(xpos, xquat, sd, phase, swing, ROOT, TIPS, **kw)


def _rollout(tripod, flags, rho, sigma, n_steps, corr=None, dtype=np.float64, stance=None, **kw):
    cpg = tripod[0]
    n = len(flags)
    corr = np.linspace(-0.03, 0.03, cpg.cycle.shape[1]).astype(np.float32) if corr is None else corr
    return spec.rollout(cpg.cycle, cpg.leg_of_dof, cpg_spec.reset_phases(n), np.ones((n, 6)), np.ones((n, 2)), n_steps, timestep=DT,
                        flags=flags, retraction=rho, stumbling=sigma, corr=corr, stance=stance, adhesion=(20.0, 1.0), dtype=dtype, **kw)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_without_a_flag_it_is_the_cpg(tripod, dtype):
    """No flag, rho = sigma = 0: rows (adhesion columns included), phases and magnitudes equal ``cpg_spec.rollout`` bit for bit."""
    cpg, _, _, stance = tripod
    n = 3
    drive = np.array([[1.0, 0.4], [0.0, 1.0], [-1.0, 1.2]])
    start = np.mod(cpg_spec.reset_phases(n) + 0.13, 1.0)
    zeros = np.zeros((n, 6))
    got = spec.rollout(cpg.cycle, cpg.leg_of_dof, start, np.ones((n, 6)), drive, 70, timestep=DT, flags=np.zeros((n, 6), np.uint8),
                       retraction=zeros, stumbling=zeros, corr=np.full(42, 0.03, np.float32), stance=stance, adhesion=(20.0, 1.0), dtype=dtype)
    ref = cpg_spec.rollout(cpg.cycle, cpg.leg_of_dof, start, np.ones((n, 6)), drive, 70, timestep=DT, stance=stance, adhesion=(20.0, 1.0),
                           dtype=dtype)
    for a, b in zip((got[0], got[1], got[2], got[4], got[5]), ref):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert not got[3].any() and not got[6].any() and not got[7].any()


def test_the_deepest_leg_retracts_only_beyond_the_threshold(tripod):
    """h3 is the third largest h: the deepest leg retracts when it is more than the threshold below it, not when it is only below
    the second; equal depths go to the lowest leg index; at most one leg per world."""
    swing = ~tripod[3]
    base = np.array([0.50, 0.52, 0.48, 0.51, 0.49, 0.50])             # once leg 4 is the deepest, the third largest is 0.51
    h = np.tile(base, (6, 1))
    h[0, 4] = 0.50 + THR_H + 1e-3          # beyond the fourth largest + threshold, not beyond the third: no
    h[1, 4] = 0.51 + THR_H + 1e-3          # beyond the third largest + threshold
    h[2, 4] = 0.51 + THR_H - 1e-3          # just short
    h[3, 2] = h[3, 5] = 0.7                # a tie of two deep legs: the lower index
    h[4] = 0.5                             # all equal
    h[5, 0] = 0.9; h[5, 1] = 0.88          # two deep legs: the third largest is 0.51, only the deepest retracts
    flags = _decide(*_inputs(6, h), cpg_spec.reset_phases(6), swing)
    expected = np.zeros((6, 6), np.uint8)
    expected[1, 4] = expected[3, 2] = expected[5, 0] = spec.RETRACT
    assert np.array_equal(flags, expected)
    assert np.array_equal(_decide(*_inputs(6, h), cpg_spec.reset_phases(6), swing, dtype=np.float32), expected)
    assert (np.count_nonzero(flags & spec.RETRACT, axis=1) <= 1).all()


def test_rho_ramps_by_up_stops_at_the_cap_and_decays_to_zero(tripod):
    up_r, down_r, up_s, down_s = spec.increments(DT)
    assert (up_r, down_r, up_s, down_s) == tuple(np.float32(v) for v in (0.08, 0.07, 0.22, 0.18))
    flags = np.zeros((1, 6), np.uint8); flags[0, 2] = spec.RETRACT
    zeros = np.zeros((1, 6))
    out = _rollout(tripod, flags, zeros, zeros, 40, dtype=np.float32)
    nets, rho = out[3], out[6]
    ramp = np.zeros(41, np.float32)
    for k in range(40):
        ramp[k + 1] = np.float32(ramp[k] + up_r)
    assert nets.dtype == np.float32 and np.array_equal(nets[0, :, 2], ramp[:40]) and rho[0, 2] == ramp[40]
    assert not np.delete(nets[0], 2, axis=1).any()
    # the cap: from 79.95 one step of 0.08 stops at exactly 80, and stays
    near = zeros.copy(); near[0, 2] = 79.95
    capped = _rollout(tripod, flags, near, zeros, 3, dtype=np.float32)
    assert np.array_equal(capped[3][0, :, 2], np.array([np.float32(79.95), 80.0, 80.0], np.float32)) and capped[6][0, 2] == 80.0
    # decay: 0.2 -> 0.13 -> 0.06 -> exactly 0, and stays
    start = zeros.copy(); start[0, 2] = 0.2
    decay = _rollout(tripod, np.zeros((1, 6), np.uint8), start, zeros, 5, dtype=np.float32)
    a = np.float32(0.2); b = np.float32(a - down_r); c = np.float32(b - down_r)
    assert np.array_equal(decay[3][0, :, 2], np.array([a, b, c, 0.0, 0.0], np.float32)) and decay[6][0, 2] == 0.0
    # a custom cap and rates
    custom = _rollout(tripod, flags, zeros, zeros, 4, dtype=np.float32, retraction_rates=(5000.0, 1.0), max_correction=1.25)
    assert np.array_equal(custom[3][0, :, 2], np.array([0.0, 0.5, 1.0, 1.25], np.float32))


def test_retraction_takes_precedence_and_the_adhesion_column_is_off(tripod):
    """net = rho while rho > 0, else sigma; the target gains net * corr in two roundings; the adhesion column is ``off`` while
    net > 0 and the CPG's value otherwise."""
    cpg, _, _, stance = tripod
    rho = np.zeros((2, 6)); sigma = np.zeros((2, 6))
    rho[0, 1] = 0.14; sigma[0, 1] = 3.0        # leg 1: rho for two steps (0.14, 0.07), then sigma
    sigma[0, 4] = 0.36                         # leg 4: sigma decays 0.36, 0.18, 0
    corr = np.linspace(-0.03, 0.03, 42).astype(np.float32)
    flags = np.zeros((2, 6), np.uint8)
    out = _rollout(tripod, flags, rho, sigma, 4, corr=corr, dtype=np.float32, stance=stance)
    rows, nets = out[0], out[3]
    ref = cpg_spec.rollout(cpg.cycle, cpg.leg_of_dof, cpg_spec.reset_phases(2), np.ones((2, 6)), np.ones((2, 2)), 4, timestep=DT,
                           stance=stance, adhesion=(20.0, 1.0), dtype=np.float32)[0]
    f = np.float32
    s1 = [f(3.0), f(f(3.0) - f(0.18)), f(f(f(3.0) - f(0.18)) - f(0.18)), f(f(f(f(3.0) - f(0.18)) - f(0.18)) - f(0.18))]
    assert np.array_equal(nets[0, :, 1], np.array([f(0.14), f(f(0.14) - f(0.07)), s1[2], s1[3]], f))
    assert np.array_equal(nets[0, :, 4], np.array([f(0.36), f(f(0.36) - f(0.18)), 0.0, 0.0], f))
    lod = cpg.leg_of_dof
    expect = (ref[..., :42] + (nets[:, :, lod] * corr[None, None, :]).astype(f)).astype(f)
    assert np.array_equal(rows[..., :42], expect) and not np.array_equal(rows[0, :, :42], ref[0, :, :42])
    assert np.array_equal(rows[1], ref[1])                                  # the world without a correction
    adh, adh_ref = rows[..., 42:], ref[..., 42:]
    assert (adh[nets > 0] == 1.0).all() and np.array_equal(adh[nets == 0], adh_ref[nets == 0])
    assert (adh_ref[0, :, 1] == 20.0).any() or (adh_ref[0, :, 4] == 20.0).any()     # (the override is seen: a stance leg)


def test_stumbling_fires_only_in_swing_bins(tripod):
    """One world per phase bin, every leg pushed backwards beyond the threshold: the flags are the swing table's row.  No flag
    without contact (found = 0), with a force short of the threshold, or with the push along another axis; a yawed body turns the
    axis the push is measured on; a contact-frame sensor is rebuilt with the third axis n x t1."""
    stance = tripod[3]
    swing = ~stance
    n_bins = len(swing)
    phase = np.tile(((np.arange(n_bins) + 0.5) / n_bins)[:, None], (1, 6))
    back = np.zeros((n_bins, 6, 3)); back[..., 0] = -1.2 * THR_F
    flags = _decide(*_inputs(n_bins, force=back), phase, swing)
    assert np.array_equal(flags, swing.astype(np.uint8) * spec.STUMBLE) and swing.any() and stance.any()
    assert np.array_equal(_decide(*_inputs(n_bins, force=back), phase, swing, dtype=np.float32), flags)
    assert not _decide(*_inputs(n_bins, force=back, found=0.0), phase, swing).any()
    assert not _decide(*_inputs(n_bins, force=0.9 * back / 1.2), phase, swing).any()
    side = np.zeros((n_bins, 6, 3)); side[..., 1] = -5.0; side[..., 2] = 9.0
    assert not _decide(*_inputs(n_bins, force=side), phase, swing).any()
    # yaw of +90 degrees: the body's x axis is the world's y, so the sideways force now pushes it backwards
    q = (np.sqrt(0.5), 0.0, 0.0, np.sqrt(0.5))
    assert np.allclose(spec.x_axis(np.array([q])), [[0, 1, 0]], atol=1e-7)
    assert np.array_equal(_decide(*_inputs(n_bins, force=side, quat=q), phase, swing), flags)
    assert not _decide(*_inputs(n_bins, force=back, quat=q), phase, swing).any()
    # contact frame of a wall with outward normal -x (contact_frame fid 2): n = (-1, 0, 0), t1 = (0, 1, 0), t2 = n x t1 = (0, 0, -1);
    # components (3, 0.5, 0.25) are the world force (-3, 0.5, -0.25)
    xpos, xquat, sd = _inputs(n_bins, force=np.broadcast_to(np.array([3.0, 0.5, 0.25]), (n_bins, 6, 3)))
    sd = sd.reshape(n_bins, 6, 16).copy(); sd[..., 10:13] = (-1, 0, 0); sd[..., 13:16] = (0, 1, 0)
    found, F = spec.world_forces(sd.reshape(n_bins, 96), True)
    assert np.array_equal(F[0, 0], [-3.0, 0.5, -0.25])
    assert np.array_equal(_decide(xpos, xquat, sd.reshape(n_bins, 96), phase, swing, contact_frame=True), flags)
    assert not _decide(xpos, xquat, sd.reshape(n_bins, 96), phase, swing, contact_frame=False).any()


def test_the_default_correction_vectors_lift_every_leg(tripod):
    """cycle + net * corr with net = cap / 4 puts the tarsus5 origin higher in the thorax frame than the cycle alone, at every
    stance bin of every leg (forward kinematics as in ``stance_bins``).  Dofs outside the clip get 0."""
    from flygym_amd.controllers import CORRECTION_VECTORS, HybridTurningCPG
    from flygym_amd.models import make_model

    cpg, fly, model, stance = tripod
    corr = HybridTurningCPG.correction_row(cpg.actuated_dofs)
    assert corr.dtype == np.float32 and corr.shape == (42,)
    for c, d in enumerate(cpg.actuated_dofs):
        if (d.parent.link, d.child.link, d.axis.value) == ("coxa", "trochanterfemur", "pitch"):
            assert corr[c] == np.float32(CORRECTION_VECTORS[d.child.pos[1]][3])
    gain = spec.lifts(model, fly, cpg, corr, spec.CAP / 4)
    worst = [float(gain[stance[:, leg], leg].min()) for leg in range(6)]
    print("least height gain of the tarsus5 origin over the stance bins at net = cap / 4, per leg:", [round(v, 3) for v in worst])
    assert min(worst) > 0.0
    custom = HybridTurningCPG.correction_row(cpg.actuated_dofs, {"m": (1, 2, 3, 4, 5, 6, 7)})
    mid = [c for c, d in enumerate(cpg.actuated_dofs) if d.child.pos[1] == "m"]
    assert sorted(custom[mid].tolist()) == sorted([1, 2, 3, 4, 5, 6, 7] * 2)
    assert np.array_equal(np.delete(custom, mid), np.delete(corr, mid))
    with pytest.raises(ValueError):
        HybridTurningCPG.correction_row(cpg.actuated_dofs, {"f": (1, 2, 3)})
    full = make_model(joints_preset="all_possible")[0].get_actuated_jointdofs_order("position")
    wide = HybridTurningCPG.correction_row(full)
    assert wide.shape == (len(full),) and np.count_nonzero(wide) == np.count_nonzero(corr) and len(full) > 42


def test_abi_of_the_hybrid_rules():
    from flygym_amd import _native
    from flygym_amd.controllers import _CpgHybridParams, HybridTurningCPG, TurningCPG, __all__ as exported

    _native.build()
    lib = _native.lib()
    assert ctypes.sizeof(_CpgHybridParams) == lib.nmf_cpg_hybrid_params_size() == 28
    header = (_native.INCLUDE / "nmf.h").read_text()
    body = re.search(r"typedef struct nmf_cpg_hybrid_params \{(.*?)\} nmf_cpg_hybrid_params;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [name.strip() for decl in re.findall(r"float ([^;]+);", body) for name in decl.split(",")]
    assert declared == [name for name, _ in _CpgHybridParams._fields_]
    assert all(ty is ctypes.c_float for _, ty in _CpgHybridParams._fields_)
    for name in ("nmf_cpg_hybrid_params_size", "nmf_cpg_hybrid_enable", "nmf_cpg_advance_hybrid"):
        assert hasattr(lib, name) and name in _native.exported_symbols(), name
    for name, value in (("NMF_CPG_RETRACTION", 3), ("NMF_CPG_STUMBLING", 4), ("NMF_CPG_RULE_FLAGS", 5)):
        assert re.search(rf"#define {name} {value}\b", header), name
    assert "HybridTurningCPG" in exported and issubclass(HybridTurningCPG, TurningCPG)
    # refusals that need no device
    assert lib.nmf_cpg_advance_hybrid(None, 1, None, 1, None) != 0 and b"null controller" in lib.nmf_last_error()
    assert lib.nmf_cpg_hybrid_enable(None, None, None, None, 0, None) != 0 and b"null controller" in lib.nmf_last_error()
