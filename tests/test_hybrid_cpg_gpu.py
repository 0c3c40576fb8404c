"""The hybrid turning controller on the GPU (``flygym_amd/csrc/nmf_cpg.hip``, ``flygym_amd.controllers.HybridTurningCPG``) against its
numpy specification ``tests/hybrid_spec.py``.

The rules' inputs are synthetic: after ``sim.reset()`` the tests write chosen values into the zero-copy views ``seg_xpos``,
``seg_xquat`` and ``sensordata`` of the batch and call ``advance``; nothing steps in between, so the inputs are exactly known.  They
keep margins — every h difference at least 1e-3 from the threshold, every force at least 1 % — so float32 and float64 cannot
decide differently, and no case is excluded from any comparison."""
import ctypes
import functools

import numpy as np
import pytest

import cpg_spec
import hybrid_spec as spec

pytestmark = pytest.mark.gpu

N = 21                                                   # three workgroups of ten worlds, the last holding one
TABLE_STEPS = 64
LAUNCHES = (1, 33, 20, 64)                               # 33 crosses the 32-step pass, 64 is two full passes
FLOOR = 1.9e-6                                           # 4 float32 ulp at 4 rad (the row bar of test_turning_cpg_gpu.py)
ADHESION = (20.0, 1.0)
THR_H, THR_F = 0.05, 2.0
# The adhesion columns and the swing test are step functions of the phase, so the inputs keep a margin there too: the start phases
# and drives (the seed) are chosen such that no phase of the float64 specification comes within 2.5e-7 cycles of a bin edge — ten
# times the kernel's phase error over the 400 steps of test_turning_cpg_gpu.py (2.5e-8, profiles/turning_cpg_parity.txt) and three
# times the distance of the two flavours of the specification there (8.6e-8).  The parity test asserts it.
EDGE_MARGIN = 2.5e-7
SEED = 20241022
KEYS = ("qpos", "qvel", "ctrl", "qacc_warmstart", "seg_xpos", "seg_xquat", "site_xpos", "actuator_force", "sensordata", "time",
        "stats", "qacc", "stats_sum", "contact_geom", "act")


@pytest.fixture
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch


@functools.lru_cache(maxsize=None)
def _batch(n=N, frame="world", copy=0, sensors=True):
    from flygym_amd import HIPSimulation, make_model
    from flygym_amd.compose import FlatGroundWorld
    from flygym_amd.utils.math import Rotation3D

    fly, world, _ = make_model()
    if not sensors:
        world = FlatGroundWorld()
        world.add_fly(fly, (0, 0, 0.8), Rotation3D("quat", (1, 0, 0, 0)), add_ground_contact_sensors=False)
    world.semantics.sensor_frame = frame
    sim = HIPSimulation(world, n_worlds=n, device=0)
    sim.set_leg_adhesion_states(fly.name, np.ones((n, 6), dtype=np.float32))
    return sim, fly


def _hybrid(sim, fly, adhesion=ADHESION, **kw):
    from flygym_amd.controllers import HybridTurningCPG

    kw = dict(dict(retraction_threshold=THR_H, stumbling_force_threshold=THR_F, table_steps=TABLE_STEPS), **kw)
    return HybridTurningCPG(sim, fly.name, adhesion=adhesion, **kw)


def _inputs(rng, cpg, base, phase, contact, quiet=False):
    """Inputs of one launch for the 21 worlds (numpy float32, shaped like the batch's views), from the reset pose ``base``:
    worlds 0-2 nothing, 3-8 retraction of leg w - 3, 9 stumbling of one swinging leg, 10-11 of every swinging leg, 12-13 and 20 both
    rules (13: on the same leg), 14 two equally deep legs, 15 a leg 2e-3 short of the threshold, 16 forces 2 % short of theirs,
    17 a force on stance legs only, 18 a force without contact, 19 a yawed body pushed along its own x axis."""
    xpos, xquat, sd = (np.array(a, dtype=np.float32) for a in base)
    n = len(phase)
    nseg = xpos.shape[1] // 3
    xpos, xquat, sd = xpos.reshape(n, nseg, 3), xquat.reshape(n, nseg, 4), np.zeros((n, 6, 16), dtype=np.float32)
    root, tips = cpg.root_seg, cpg.tip_seg
    h = rng.uniform(1.0, 1.02, (n, 6))                   # spread 0.02: nobody retracts
    swinging = cpg.swing.astype(bool)[spec.start_bins(phase, cpg.n_bins), np.arange(6)[None, :]]
    push = np.zeros((n, 6))                              # F . xhat in units of the threshold
    found = np.ones((n, 6))
    yaw = np.zeros(n)
    if not quiet:
        third = lambda w, leg: np.sort(np.delete(h[w], leg))[-2]          # the third largest once ``leg`` is the deepest
        for w in range(3, 9):
            h[w, w - 3] = third(w, w - 3) + THR_H + rng.uniform(2e-3, 0.3)
        first_swing = [int(np.argmax(swinging[w])) if swinging[w].any() else 0 for w in range(n)]
        push[9, first_swing[9]] = -rng.uniform(1.02, 3.0)
        push[10] = -rng.uniform(1.02, 3.0, 6)
        push[11] = -rng.uniform(1.02, 3.0, 6)
        for w, leg in ((12, 1), (13, first_swing[13]), (20, 5)):
            h[w, leg] = third(w, leg) + THR_H + rng.uniform(2e-3, 0.3)
            push[w] = -rng.uniform(1.02, 3.0, 6)
        h[14, 2] = h[14, 4] = 1.5
        h[15, 3] = third(15, 3) + THR_H - 2e-3
        push[16] = -0.98
        push[17] = np.where(swinging[17], 0.5, -2.5)
        push[18] = -2.5; found[18] = 0.0
        push[19] = -rng.uniform(1.02, 3.0, 6); yaw[19] = 1.1
        found[10] = 2.0
    z_root = rng.uniform(1.4, 1.6, n)
    xpos[:, root, 2] = z_root
    xpos[:, tips, 2] = z_root[:, None] - h
    xquat[:, root] = np.stack([np.cos(yaw / 2), 0 * yaw, 0 * yaw, np.sin(yaw / 2)], axis=1)
    ax = spec.x_axis(xquat[:, root])                                                    # (n, 3)
    side = np.stack([-ax[:, 1], ax[:, 0], 0 * ax[:, 0]], axis=1)
    F = (push * THR_F)[:, :, None] * ax[:, None, :] + rng.uniform(-5, 5, (n, 6, 1)) * side[:, None, :]
    F[..., 2] += rng.uniform(0, 9, (n, 6))
    if quiet:
        F[:] = 0.0
    nrm, tan = np.array([0.0, 0.0, 1.0]), np.array([0.0, 1.0, 0.0])
    if contact:                                          # the components along (n, t1, n x t1): a wall facing -x for odd legs
        nrm = np.where(np.arange(6)[:, None] % 2 == 1, np.array([-1.0, 0.0, 0.0]), nrm)
        tan = np.broadcast_to(tan, (6, 3))
        frame = np.stack([nrm, tan, np.cross(nrm, tan)], axis=1)                        # (6, 3 axes, 3)
        F = np.einsum("lak,wlk->wla", frame, F)
    sd[..., 0], sd[..., 1:4], sd[..., 10:13], sd[..., 13:16] = found, F, nrm, tan
    sd[..., 4:10] = rng.uniform(-1, 1, (n, 6, 6))                                       # torque and position: not read
    return xpos.reshape(n, -1), xquat.reshape(n, -1), sd.reshape(n, 96)


def _base(torch, sim):
    sim.reset()
    torch.cuda.synchronize()
    return tuple(sim.field(k).cpu().numpy().copy() for k in ("seg_xpos", "seg_xquat", "sensordata"))


def _write(torch, sim, inputs, worlds=None):
    for key, a in zip(("seg_xpos", "seg_xquat", "sensordata"), inputs):
        sim.field(key).copy_(torch.as_tensor(a if worlds is None else a[worlds], device=sim.device))


def _spec_launch(cpg, inputs, state, drive, n_steps, contact, dtype):
    th, r, rho, sigma = state
    flags = spec.decide(*inputs, th, cpg.swing, cpg.root_seg, cpg.tip_seg, retraction_threshold=cpg.retraction_threshold,
                        stumbling_force_threshold=cpg.stumbling_force_threshold, contact_frame=contact, dtype=dtype)
    rows, phases, _, nets, th, r, rho, sigma = spec.rollout(
        cpg.cycle, cpg.leg_of_dof, th, r, drive, n_steps, timestep=cpg.timestep, flags=flags, retraction=rho, stumbling=sigma, corr=cpg.corr,
        retraction_rates=cpg.retraction_rates, stumbling_rates=cpg.stumbling_rates, max_correction=cpg.max_correction,
        frequency=cpg.frequency, coupling=cpg.coupling, convergence=cpg.convergence, stance=cpg.stance, adhesion=cpg.adhesion or (1.0, 0.0),
        dtype=dtype)
    return flags, rows, phases, (th, r, rho, sigma), nets


def _start(rng):
    """Perturbed start phases, and rules' states that reach the cap (world 3's rho, world 10's sigma) and zero inside a launch."""
    start = np.mod(cpg_spec.reset_phases(N) + rng.uniform(-0.3, 0.3, (N, 6)), 1.0)
    rho, sigma = np.zeros((N, 6), np.float32), np.zeros((N, 6), np.float32)
    rho[3, 0] = 79.0; sigma[10] = 79.9; rho[1, 2] = 1.0; sigma[2, 4] = 3.0; sigma[1, 2] = 9.0
    return start, rho, sigma


@pytest.mark.parametrize("frame", ["world", "contact"])
def test_parity_with_the_specification(torch_mod, frame):
    """21 worlds, launches of 1, 33, 20 and 64 steps with fresh inputs and drives before each, sensors reporting in the world frame
    and in the contact frame.  ``rule_flags``, ``retraction`` and ``stumbling`` equal the float32 specification bit for bit after
    every launch, the adhesion entries are all equal; the position columns lie within max(4 x the largest |spec32 - spec64| on these
    inputs, 1.9e-6 rad) of the float64 specification, the phases by the same rule in cycles, the magnitudes within 4 float32 ulp.
    The correction itself adds no error: a ``TurningCPG`` on the same batch, given the same phases and drives, writes the CPG part v
    of every row, and every position entry equals fl(v + fl(net corr)) bit for bit with the specification's net — the product and
    the sum rounded separately; the inputs hold entries that a fused multiply-add would round differently.
    Prints its figures with ``-s``."""
    torch = torch_mod
    from flygym_amd.controllers import TurningCPG

    contact = frame == "contact"
    sim, fly = _batch(frame=frame)
    rng = np.random.default_rng(SEED)
    start, rho0, sigma0 = _start(rng)
    base = _base(torch, sim)
    seen = np.zeros(4, dtype=int)
    with _hybrid(sim, fly) as cpg, TurningCPG(sim, fly.name, adhesion=ADHESION, table_steps=TABLE_STEPS) as plain:
        assert cpg.n_act == 48 and tuple(cpg.table.shape) == (N, TABLE_STEPS, 48)
        assert cpg.rule_flags.dtype == torch.uint8 and tuple(cpg.rule_flags.shape) == (N, 6)
        assert cpg.retraction.dtype == torch.float32 and tuple(cpg.stumbling.shape) == (N, 6)
        assert bool((cpg.retraction == 0).all()) and bool((cpg.stumbling == 0).all()) and bool((cpg.rule_flags == 0).all())
        cpg.phase.copy_(torch.as_tensor(start, device=sim.device))
        plain.phase.copy_(torch.as_tensor(start, device=sim.device))
        cpg.retraction.copy_(torch.as_tensor(rho0, device=sim.device))
        cpg.stumbling.copy_(torch.as_tensor(sigma0, device=sim.device))
        s64 = (start.copy(), np.ones((N, 6)), rho0.astype(np.float64), sigma0.astype(np.float64))
        s32 = (start.copy(), np.ones((N, 6), np.float32), rho0.copy(), sigma0.copy())
        spec_rows = spec_phase = row_err = phase_err = mag_ulps = top_rho = top_sigma = 0.0
        edge = 1.0
        fma_would_differ = 0
        corr32, lod = np.asarray(cpg.corr, dtype=np.float32), np.asarray(cpg.leg_of_dof)
        ulp = lambda v: np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)
        for k, n_steps in enumerate(LAUNCHES):
            drive = rng.uniform(-1.0, 1.5, (N, 2)).astype(np.float32)
            inputs = _inputs(rng, cpg, base, s32[0], contact)
            _write(torch, sim, inputs)
            cpg.set_drive(drive); plain.set_drive(drive)
            got = cpg.advance(n_steps)[:, :n_steps].cpu().numpy()
            cpg_part = plain.advance(n_steps)[:, :n_steps, :42].cpu().numpy()
            assert torch.equal(cpg.phase, plain.phase) and torch.equal(cpg.magnitude, plain.magnitude), k   # the oscillators are not modified
            g_flags, g_rho, g_sigma = (v.cpu().numpy() for v in (cpg.rule_flags, cpg.retraction, cpg.stumbling))
            g_phase, g_mag = cpg.phase.cpu().numpy(), cpg.magnitude.cpu().numpy()
            f64, rows64, ph64, s64, _ = _spec_launch(cpg, inputs, s64, drive, n_steps, contact, np.float64)
            f32, rows32, _, s32, nets32 = _spec_launch(cpg, inputs, s32, drive, n_steps, contact, np.float32)
            assert np.array_equal(f32, f64), k                                   # the margins: both flavours decide alike
            x = ph64 * cpg.n_bins
            edge = min(edge, float((np.abs(x - np.round(x)) / cpg.n_bins).min()))
            assert np.array_equal(rows32[..., 42:], rows64[..., 42:]), k
            assert np.array_equal(g_flags, f32), (k, g_flags, f32)
            assert g_rho.dtype == np.float32 and np.array_equal(g_rho, s32[2]) and np.array_equal(g_sigma, s32[3]), k
            assert np.array_equal(got[..., 42:], rows32[..., 42:]), k
            assert np.isfinite(got).all()
            assert nets32.dtype == np.float32 and cpg_part.dtype == np.float32
            product = nets32[:, :, lod] * corr32[None, None, :]                  # float32: the first rounding
            assert np.array_equal(got[..., :42], cpg_part + product), k          # the second
            fused = (cpg_part.astype(np.float64) + nets32[:, :, lod].astype(np.float64) * corr32.astype(np.float64)).astype(np.float32)
            fma_would_differ += int((fused != cpg_part + product).sum())
            top_rho, top_sigma = max(top_rho, float(s32[2].max())), max(top_sigma, float(s32[3].max()))
            for bit in (1, 2, 3):
                seen[bit] += int((f32 == bit).sum())
            spec_rows = max(spec_rows, float(np.abs(rows32[..., :42].astype(np.float64) - rows64[..., :42]).max()))
            spec_phase = max(spec_phase, float(np.abs(cpg_spec.wrap(s32[0] - s64[0])).max()))
            row_err = max(row_err, float(np.abs(got[..., :42].astype(np.float64) - rows64[..., :42]).max()))
            phase_err = max(phase_err, float(np.abs(cpg_spec.wrap(g_phase - s64[0])).max()))
            mag_ulps = max(mag_ulps, float((np.abs(g_mag.astype(np.float64) - s64[1]) / ulp(s64[1])).max()))
            exact = float((got[..., :42] == rows32[..., :42]).mean())
        row_bar, phase_bar = max(4.0 * spec_rows, FLOOR), max(4.0 * spec_phase, FLOOR)
        print(f"hybrid cpg parity, {frame} frame: rows spec32-vs-spec64 {spec_rows:.3e} rad, bar {row_bar:.3e}, kernel {row_err:.3e} "
              f"(last launch: {exact:.4f} of the position entries equal spec32 bitwise); phases bar {phase_bar:.3e}, kernel {phase_err:.3e}; "
              f"magnitudes {mag_ulps:.2f} ulp (bar 4); position entries equal fl(TurningCPG's + fl(net corr)) bitwise: all, a fused multiply-add "
              f"would change {fma_would_differ}; flags seen: retract {seen[1]}, stumble {seen[2]}, both {seen[3]}")
        assert seen[1] >= 6 * len(LAUNCHES) and seen[2] >= len(LAUNCHES) and seen[3] >= 1
        assert edge > EDGE_MARGIN, edge
        assert top_rho == 80.0 and top_sigma == 80.0                                 # the cap was reached inside a launch
        assert fma_would_differ > 0
        assert row_err <= row_bar and phase_err <= phase_bar and mag_ulps <= 4.0


def test_nothing_fires_it_is_the_turning_cpg(torch_mod):
    """With inputs that fire nothing, table, phase and magnitude are bitwise those of a ``TurningCPG`` on the same batch given the
    same phases and drives, over launches of 1, 33, 20 and 64 steps."""
    torch = torch_mod
    from flygym_amd.controllers import TurningCPG

    sim, fly = _batch()
    rng = np.random.default_rng(5)
    start = _start(rng)[0]
    base = _base(torch, sim)
    with _hybrid(sim, fly) as hyb, TurningCPG(sim, fly.name, adhesion=ADHESION, table_steps=TABLE_STEPS) as plain:
        for c in (hyb, plain):
            c.phase.copy_(torch.as_tensor(start, device=sim.device))
        for n_steps in LAUNCHES:
            _write(torch, sim, _inputs(rng, hyb, base, hyb.phase.cpu().numpy(), False, quiet=True))
            drive = rng.uniform(-1.0, 1.5, (N, 2)).astype(np.float32)
            hyb.set_drive(drive); plain.set_drive(drive)
            a, b = hyb.advance(n_steps), plain.advance(n_steps)
            assert torch.equal(a[:, :n_steps], b[:, :n_steps]), n_steps
            assert torch.equal(hyb.phase, plain.phase) and torch.equal(hyb.magnitude, plain.magnitude), n_steps
            assert not bool(hyb.rule_flags.any()) and not bool(hyb.retraction.any()) and not bool(hyb.stumbling.any())
        assert bool(torch.isfinite(hyb.table).all()) and not bool((hyb.table[:, :, :42] == 0).all())


def test_a_world_does_not_depend_on_its_place_in_the_batch(torch_mod):
    """Worlds 20 (alone in its workgroup), 7 and 12 of the 21-world batch and the same worlds at indices 0, 1, 2 of a 3-world batch:
    table, phase, magnitude, retraction, stumbling and flags are bitwise the same over launches of 33 and 20 steps."""
    torch = torch_mod
    big_sim, fly = _batch()
    small_sim, small_fly = _batch(n=3)
    worlds = np.array([20, 7, 12])
    rng = np.random.default_rng(11)
    start, rho0, sigma0 = _start(rng)
    base = _base(torch, big_sim)
    _base(torch, small_sim)
    with _hybrid(big_sim, fly) as big, _hybrid(small_sim, small_fly) as small:
        for c, sel in ((big, slice(None)), (small, worlds)):
            c.phase.copy_(torch.as_tensor(start[sel], device=c.sim.device))
            c.retraction.copy_(torch.as_tensor(rho0[sel] + 0.5, device=c.sim.device))
            c.stumbling.copy_(torch.as_tensor(sigma0[sel], device=c.sim.device))
        fired = 0
        for n_steps in (33, 20):
            inputs = _inputs(rng, big, base, big.phase.cpu().numpy(), False)
            drive = rng.uniform(-1.0, 1.5, (N, 2)).astype(np.float32)
            _write(torch, big_sim, inputs); _write(torch, small_sim, inputs, worlds)
            big.set_drive(drive); small.set_drive(drive[worlds])
            tb, ts = big.advance(n_steps), small.advance(n_steps)
            sel = torch.as_tensor(worlds, device=big_sim.device)
            assert torch.equal(ts[:, :n_steps], tb[sel, :n_steps]), n_steps
            for name in ("phase", "magnitude", "retraction", "stumbling", "rule_flags"):
                assert torch.equal(getattr(small, name), getattr(big, name)[sel]), (n_steps, name)
            fired += int(small.rule_flags.count_nonzero())
        assert fired >= 4


def test_masked_reset(torch_mod):
    """After a launch in which both rules fire, ``reset(mask)`` zeroes rho / sigma / flags of the masked worlds only and puts their
    oscillators back on the tripod; the others continue bitwise like a controller that was never reset."""
    torch = torch_mod
    sim, fly = _batch()
    rng = np.random.default_rng(3)
    start = _start(rng)[0]
    base = _base(torch, sim)
    with _hybrid(sim, fly) as cpg, _hybrid(sim, fly) as twin:
        for c in (cpg, twin):
            c.phase.copy_(torch.as_tensor(start, device=sim.device))
        _write(torch, sim, _inputs(rng, cpg, base, start, False))
        cpg.advance(40); twin.advance(40)
        before = {k: getattr(cpg, k).clone() for k in ("phase", "magnitude", "retraction", "stumbling", "rule_flags")}
        mask = torch.arange(N, device=sim.device) % 2 == 1
        assert bool(before["retraction"][mask].any()) and bool(before["stumbling"][mask].any()) and bool(before["rule_flags"][mask].any())
        assert bool(before["retraction"][~mask].any()) and bool(before["stumbling"][~mask].any())
        cpg.reset(mask.cpu().numpy())
        torch.cuda.synchronize()
        for k in ("retraction", "stumbling", "rule_flags"):
            assert not bool(getattr(cpg, k)[mask].any()), k
        for k, was in before.items():
            assert torch.equal(getattr(cpg, k)[~mask], was[~mask]), k
        assert np.abs(cpg.phase[mask].cpu().numpy() - cpg_spec.reset_phases(N)[mask.cpu().numpy()]).max() < 1e-15
        _write(torch, sim, _inputs(rng, cpg, base, twin.phase.cpu().numpy(), False))
        a, b = cpg.advance(33), twin.advance(33)
        assert torch.equal(a[~mask, :33], b[~mask, :33]) and not torch.equal(a[mask, :33], b[mask, :33])
        for k in before:
            assert torch.equal(getattr(cpg, k)[~mask], getattr(twin, k)[~mask]), k
        cpg.reset()
        torch.cuda.synchronize()
        assert not bool(cpg.retraction.any()) and not bool(cpg.stumbling.any()) and not bool(cpg.rule_flags.any())


def test_one_control_tick_is_one_captured_graph(torch_mod):
    """Drive copy + ``advance(20)`` + ``step_replay`` captured with ``torch.cuda.graph`` on a flat world with real physics; the
    thresholds are zero so that the rules fire from real sensor values.  Two replays equal two eager ticks bitwise."""
    torch = torch_mod
    ticks = []
    for copy in (1, 2):
        sim, fly = _batch(copy=copy)
        sim.reset()
        sim.warmup()
        cpg = _hybrid(sim, fly, retraction_threshold=0.0, stumbling_force_threshold=0.0)
        staged = torch.ones((N, 2), dtype=torch.float32, device=sim.device)

        def tick(cpg=cpg, sim=sim, staged=staged):
            cpg.drive.copy_(staged)
            sim.step_replay(cpg.advance(20), cpg.act_ids, 0, 20)

        torch.zeros_like(cpg.drive).copy_(staged)                # (torch's own kernels are loaded before the capture)
        ticks.append((cpg, sim, staged, tick))
    torch.cuda.synchronize()
    (c0, s0, d0, eager), (c1, s1, d1, captured) = ticks
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured()
    rng = np.random.default_rng(9)
    fired = 0
    for k in range(2):
        new = torch.as_tensor(rng.uniform(0.4, 1.2, (N, 2)).astype(np.float32), device=s0.device)
        d0.copy_(new); d1.copy_(new)
        g.replay()
        eager()
        torch.cuda.synchronize()
        for name in ("table", "phase", "magnitude", "drive", "retraction", "stumbling", "rule_flags"):
            assert torch.equal(getattr(c0, name), getattr(c1, name)), (k, name)
        for key in KEYS:
            assert torch.equal(s0.field(key), s1.field(key)), (k, key)
        fired += int(c0.rule_flags.count_nonzero())
    assert fired > 0 and bool(c0.retraction.any()) and bool(torch.isfinite(s0.field("qpos")).all())
    c0.close(); c1.close()


def test_refusals_leave_the_state_untouched(torch_mod):
    torch = torch_mod
    from flygym_amd import _native
    from flygym_amd.controllers import TurningCPG, _CpgHybridParams

    lib = _native.lib()
    sim, fly = _batch()
    hyb = _hybrid(sim, fly)
    plain = TurningCPG(sim, fly.name, adhesion=ADHESION, table_steps=TABLE_STEPS)
    state = lambda c: [getattr(c, k).clone() for k in ("phase", "magnitude", "drive", "table")]
    before_h, before_p = state(hyb) + [hyb.retraction.clone(), hyb.stumbling.clone(), hyb.rule_flags.clone()], state(plain)

    def refused(rc, text):
        assert rc != 0 and text in lib.nmf_last_error(), (rc, lib.nmf_last_error())

    table = plain.table.data_ptr()
    refused(lib.nmf_cpg_advance_hybrid(plain._h, 20, table, TABLE_STEPS, None), b"not enabled")
    assert not lib.nmf_cpg_field_ptr(plain._h, 3, None) and b"not enabled" in lib.nmf_last_error()
    par, corr, swing, tips = hyb._hybrid_params, hyb.corr, hyb.swing, hyb.tip_seg
    enable = lambda h, p=par, c=corr, root=hyb.root_seg, t=tips: lib.nmf_cpg_hybrid_enable(
        h, ctypes.byref(p), c.ctypes.data, swing.ctypes.data, root, t.ctypes.data)
    refused(enable(hyb._h), b"already enabled")
    nseg = sim.model.nseg
    refused(enable(plain._h, root=nseg), b"root_seg")
    refused(enable(plain._h, root=-1), b"root_seg")
    bad_tips = tips.copy(); bad_tips[4] = nseg
    refused(enable(plain._h, t=bad_tips), b"tip_seg[4]")
    for field in ("retraction_threshold", "stumbling_force_threshold", "retraction_up", "retraction_down", "stumbling_up",
                  "stumbling_down", "max_correction"):
        bad = _CpgHybridParams.from_buffer_copy(par); setattr(bad, field, -1.0)
        refused(enable(plain._h, p=bad), b"not negative")
    for value in (np.nan, np.inf):
        bad_corr = corr.copy(); bad_corr[5] = value
        refused(enable(plain._h, c=bad_corr), b"corr[5]")
    refused(lib.nmf_cpg_hybrid_enable(plain._h, None, None, None, 0, None), b"required")
    # everything nmf_cpg_advance refuses
    htable = hyb.table.data_ptr()
    for args, text in (((0, htable, TABLE_STEPS), b"n_steps"), ((TABLE_STEPS + 1, htable, TABLE_STEPS), b"n_steps"),
                       ((1, None, TABLE_STEPS), b"null table"), ((1, htable, 32), b"tables of 64 steps")):
        refused(lib.nmf_cpg_advance_hybrid(hyb._h, args[0], args[1], args[2], None), text)
    for bad in (0, TABLE_STEPS + 1):
        with pytest.raises(ValueError, match="n_steps"):
            hyb.advance(bad)
    # a batch whose model has no leg sensors
    bare_sim, bare_fly = _batch(n=3, sensors=False)
    assert int(bare_sim.model["n_sensor"][0]) == 0
    with pytest.raises(_native.NativeError, match="no leg sensors"):
        _hybrid(bare_sim, bare_fly)
    with pytest.raises(ValueError):
        _hybrid(sim, fly, correction_vectors={"f": (1, 2)})
    torch.cuda.synchronize()
    for now, was in zip(state(hyb) + [hyb.retraction, hyb.stumbling, hyb.rule_flags], before_h):
        assert torch.equal(now, was)
    for now, was in zip(state(plain), before_p):
        assert torch.equal(now, was)
    assert bool((hyb.table == 0).all()) and bool((plain.table == 0).all())
    # the refused controller still is a working TurningCPG, and can be enabled once
    assert lib.nmf_cpg_advance(plain._h, 20, table, TABLE_STEPS, None) == 0
    assert enable(plain._h) == 0
    assert lib.nmf_cpg_advance_hybrid(plain._h, 20, table, TABLE_STEPS, None) == 0
    torch.cuda.synchronize()
    hyb.close(); plain.close()
    with pytest.raises(RuntimeError, match="closed"):
        hyb.advance(1)
    assert hyb.retraction is None and hyb.rule_flags is None


def test_refused_creations_leak_nothing_and_leave_the_controller_usable(torch_mod):
    """Two worlds of the LEGS_ONLY model.  32 rounds of one refused call per handle type — a camera plan with a capsule segment out of
    range, a CPG with a leg index outside 0..5, ``nmf_cpg_hybrid_enable`` with a tip segment out of range on a live controller — each
    rejected by the host checks before any kernel runs.  Afterwards the device has no less free memory than before the rounds, to
    within the one allocation granule that a 16-byte ``torch.empty`` moves ``mem_get_info`` by here, and the live controller's next
    4 steps are a fresh controller's bit for bit."""
    torch = torch_mod
    from flygym_amd import _native
    from flygym_amd.controllers import TurningCPG
    from flygym_amd.rendering import HIPBatchRenderer

    lib = _native.lib()
    sim, fly = _batch(n=2)
    # one create / destroy of each handle type first: the runtime's pools are populated before the measurement
    cam = HIPBatchRenderer(sim, "trackcam", worlds=[0]); cam.close()
    hyb = _hybrid(sim, fly, adhesion=None); hyb.close()
    live = TurningCPG(sim, fly.name, table_steps=TABLE_STEPS)
    torch.cuda.synchronize()
    free = lambda: torch.cuda.mem_get_info(sim.device)[0]
    start = free()
    probe = torch.empty(16, dtype=torch.uint8, device=sim.device)
    granule = start - free()
    before = free()

    nseg = sim.model.nseg
    one = np.zeros(1, dtype=np.int32)
    seg = np.asarray([nseg], dtype=np.int32); geom = np.ones(7, dtype=np.float32); rgb = np.zeros(3, dtype=np.uint8)
    cyc = np.ascontiguousarray(live.cycle, dtype=np.float32)
    bad_legs = np.ascontiguousarray(live.leg_of_dof, dtype=np.int32); bad_legs[7] = 6
    bad_tips = hyb.tip_seg.copy(); bad_tips[4] = nseg
    for _ in range(32):
        assert not lib.nmf_camera_plan_create(sim._batch_h, ctypes.byref(cam._params), 1, one.ctypes.data, 1, seg.ctypes.data,
                                              geom.ctypes.data, rgb.ctypes.data, 1)
        assert b"capsule segment out of range" in lib.nmf_last_error()
        assert not lib.nmf_cpg_create(sim._batch_h, ctypes.byref(live._params), cyc.ctypes.data, bad_legs.ctypes.data, None)
        assert b"leg_of_col[7]" in lib.nmf_last_error()
        assert lib.nmf_cpg_hybrid_enable(live._h, ctypes.byref(hyb._hybrid_params), hyb.corr.ctypes.data, hyb.swing.ctypes.data,
                                         hyb.root_seg, bad_tips.ctypes.data) != 0
        assert b"tip_seg[4]" in lib.nmf_last_error()
    torch.cuda.synchronize()
    after = free()
    print(f"free device memory: {before} B before the refused calls, {after} B after; allocation granule {granule} B")
    assert after >= before - granule, (before, after, granule)
    del probe

    fresh = TurningCPG(sim, fly.name, table_steps=TABLE_STEPS)
    rows, want = live.advance(4)[:, :4], fresh.advance(4)[:, :4]
    torch.cuda.synchronize()
    assert torch.equal(rows, want) and bool(torch.isfinite(rows).all()) and bool((rows != 0).any())
    assert torch.equal(live.phase, fresh.phase) and torch.equal(live.magnitude, fresh.magnitude)
    live.close(); fresh.close()


def test_closed_loop_on_the_gapped_terrain(torch_mod):
    """21 flies on the gapped terrain, 100 ticks of 20 steps through ``HybridTurningCPG.step``: everything stays finite,
    0 <= rho, sigma <= cap, and the flags of every tick are those the specification decides from the views read before the tick.
    The views hold real values without margins, so the specification decides in float32 like the kernel — the heights and their
    order are then the kernel's own, single subtractions and comparisons, whichever two legs come close — and a flag may differ
    only where moving both thresholds by 1e-5 (absolute, and relative for the force) changes that decision: the band covers the
    order and contraction of the few float32 products behind F . xhat."""
    torch = torch_mod
    import flygym_amd.compose as C
    from flygym_amd import HIPSimulation, make_model
    from flygym_amd.utils.math import Rotation3D

    fly = make_model()[0]
    world = C.GappedTerrainWorld()
    world.add_fly(fly, (0.3, 0.2, 0.8), Rotation3D("quat", (1, 0, 0, 0)))
    sim = HIPSimulation(world, n_worlds=N, device=0)
    sim.set_leg_adhesion_states(fly.name, np.ones((N, 6), dtype=np.float32))
    sim.warmup()
    thr_f = 1.0
    counts = np.zeros(3, dtype=int)
    with _hybrid(sim, fly, adhesion=None, stumbling_force_threshold=thr_f) as cpg:
        decide = lambda views, ph, dh, df: spec.decide(*views, ph, cpg.swing, cpg.root_seg, cpg.tip_seg, retraction_threshold=THR_H + dh,
                                                       stumbling_force_threshold=thr_f * (1 + df) + df, dtype=np.float32)
        for tick in range(100):
            torch.cuda.synchronize()
            views = [sim.field(k).cpu().numpy() for k in ("seg_xpos", "seg_xquat", "sensordata")]
            phase = cpg.phase.cpu().numpy()
            cpg.step(20)
            flags = cpg.rule_flags.cpu().numpy()
            sure, maybe = decide(views, phase, 1e-5, 1e-5), decide(views, phase, -1e-5, -1e-5)
            assert not (sure & ~flags).any() and not (flags & ~maybe).any(), tick
            counts += [(flags & 1).any(axis=1).sum(), (flags & 2).any(axis=1).sum(), int((sure != maybe).sum())]
            rho, sigma = cpg.retraction.cpu().numpy(), cpg.stumbling.cpu().numpy()
            assert (rho >= 0).all() and (rho <= 80.0).all() and (sigma >= 0).all() and (sigma <= 80.0).all(), tick
        torch.cuda.synchronize()
        qpos = sim.field("qpos").cpu().numpy()
        print(f"hybrid cpg on the gapped terrain, 21 worlds x 100 ticks: world-ticks with a retraction {counts[0]}, with a stumble "
              f"{counts[1]}; decisions within 1e-5 of a threshold {counts[2]}; mean x travelled {float(qpos[:, 0].mean() - 0.3):.3f} mm")
        assert np.isfinite(qpos).all() and bool(torch.isfinite(cpg.table[:, :20]).all()) and bool(torch.isfinite(cpg.phase).all())
        assert np.isfinite(sim.field("qvel").cpu().numpy()).all()
