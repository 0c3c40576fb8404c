"""The closed-loop tripod CPG on the GPU (``flygym_amd/csrc/nmf_cpg.hip``, ``flygym_amd.controllers.TurningCPG``) against its numpy
specification ``tests/cpg_spec.py``."""
import ctypes
import functools

import numpy as np
import pytest

import cpg_spec as spec

pytestmark = pytest.mark.gpu

N = 67                                                   # prime: the last workgroup's wave is partly filled whatever the packing
LAUNCHES = (1, 20, 37, 64, 64, 64, 64, 64, 22)           # 400 steps; 37 and 22 end inside a pass, 64 takes two passes
FLOOR = 1.9e-6                                           # 4 float32 ulp at 4 rad
KEYS = ("qpos", "qvel", "ctrl", "qacc_warmstart", "seg_xpos", "seg_xquat", "site_xpos", "actuator_force", "sensordata", "time",
        "stats", "qacc", "stats_sum", "contact_geom", "act")
ADHESION = (20.0, 1.0)


@pytest.fixture
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch


@functools.lru_cache(maxsize=None)
def _batch(preset="legs_only", n=N, copy=0):
    """A settled batch of n worlds of the benchmark fly (one per preset / size / copy, shared by the tests that only need a batch
    to attach a controller to; tests that step one ask for their own copy)."""
    from flygym_amd import HIPSimulation, make_model

    fly, world, _ = make_model(joints_preset=preset)
    sim = HIPSimulation(world, n_worlds=n, device=0)
    sim.set_leg_adhesion_states(fly.name, np.ones((n, 6), dtype=np.float32))
    sim.warmup()
    return sim, fly


def _controller(preset="legs_only", adhesion=None, n=N, copy=0, **kw):
    from flygym_amd.controllers import TurningCPG

    sim, fly = _batch(preset, n, copy)
    return TurningCPG(sim, fly.name, adhesion=adhesion, **kw)


@functools.lru_cache(maxsize=None)
def _scenario():
    """Start phases perturbed per world and one drive per launch and world from a seeded generator: drawn from [-1, 1.5], worlds
    0..5 with a side at exactly 0, 6..11 at exactly 1, 12..17 negative on one side."""
    rng = np.random.default_rng(20240917)
    start = np.mod(spec.reset_phases(N) + rng.uniform(-0.3, 0.3, (N, 6)), 1.0)
    drives = rng.uniform(-1.0, 1.5, (len(LAUNCHES), N, 2)).astype(np.float32)
    drives[:, 0:3, 0] = 0.0
    drives[:, 3:6, 1] = 0.0
    drives[:, 6:9, 0] = 1.0
    drives[:, 9:12, :] = 1.0
    drives[:, 12:15, 0] = -np.abs(drives[:, 12:15, 0]) - 0.1
    drives[:, 15:18, 1] = -0.5
    start.setflags(write=False)
    drives.setflags(write=False)
    return start, drives


def _run_gpu(torch, cpg, start, drives, launches):
    """Rows of all launches (n, total, n_act) and the (phase, magnitude) after each launch, as numpy."""
    cpg.reset()
    cpg.phase.copy_(torch.as_tensor(np.array(start), device=cpg.sim.device))
    rows, states = [], []
    for k, n_steps in enumerate(launches):
        cpg.set_drive(drives[k])
        rows.append(cpg.advance(n_steps)[:, :n_steps].clone())
        states.append((cpg.phase.clone(), cpg.magnitude.clone()))
    torch.cuda.synchronize()
    return torch.cat(rows, dim=1).cpu().numpy(), [(p.cpu().numpy(), m.cpu().numpy()) for p, m in states]


def _run_spec(cpg, start, drives, launches, dtype):
    th, r = np.array(start), np.ones(start.shape, dtype=dtype)
    rows, states = [], []
    for k, n_steps in enumerate(launches):
        out, _, _, th, r = spec.rollout(cpg.cycle, cpg.leg_of_dof, th, r, drives[k], n_steps, timestep=cpg.timestep,
                                        frequency=cpg.frequency, coupling=cpg.coupling, convergence=cpg.convergence,
                                        stance=cpg.stance, adhesion=cpg.adhesion or (1.0, 0.0), dtype=dtype)
        rows.append(out)
        states.append((th, r))
    return np.concatenate(rows, axis=1), states


def _edge_distance(phase, n_bins):
    """Distance (cycles) of a phase from the nearest bin edge."""
    x = phase * n_bins
    return np.abs(x - np.round(x)) / n_bins


def _compare(label, cpg, got, states, start, drives, launches):
    """The bars of the parity test against the float64 specification; returns the figures."""
    n_pos = len(cpg.actuated_dofs)
    rows64, st64 = _run_spec(cpg, start, drives, launches, np.float64)
    rows32, st32 = _run_spec(cpg, start, drives, launches, np.float32)
    spec_rows = float(np.abs(rows32[..., :n_pos].astype(np.float64) - rows64[..., :n_pos]).max())
    spec_phase = max(float(np.abs(spec.wrap(a[0] - b[0])).max()) for a, b in zip(st32, st64))
    row_bar, phase_bar = max(4.0 * spec_rows, FLOOR), max(4.0 * spec_phase, FLOOR)
    row_err = float(np.abs(got[..., :n_pos].astype(np.float64) - rows64[..., :n_pos]).max())
    phase_err = max(float(np.abs(spec.wrap(g[0] - s[0])).max()) for g, s in zip(states, st64))
    ulp = lambda v: np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)
    mag_ulps = max(float((np.abs(g[1].astype(np.float64) - s[1]) / ulp(s[1])).max()) for g, s in zip(states, st64))
    spec_mag_ulps = max(float((np.abs(a[1].astype(np.float64) - b[1]) / ulp(b[1])).max()) for a, b in zip(st32, st64))
    line = (f"turning cpg parity {label}: rows spec32-vs-spec64 {spec_rows:.3e} rad, bar {row_bar:.3e}, kernel {row_err:.3e}; "
            f"phases spec32-vs-spec64 {spec_phase:.3e} cycles, bar {phase_bar:.3e}, kernel {phase_err:.3e}; "
            f"magnitudes spec32-vs-spec64 {spec_mag_ulps:.2f} ulp, bar 4, kernel {mag_ulps:.2f} ulp")
    shares = None
    if cpg.stance is not None:
        # the phases the rows were computed from, per step, from the float64 specification
        th, r, ph = np.array(start), np.ones(start.shape), []
        for k, n_steps in enumerate(launches):
            _, p, _, th, r = spec.rollout(cpg.cycle, cpg.leg_of_dof, th, r, drives[k], n_steps, timestep=cpg.timestep,
                                          frequency=cpg.frequency, coupling=cpg.coupling, convergence=cpg.convergence)
            ph.append(p)
        near = _edge_distance(np.concatenate(ph, axis=1), cpg.n_bins) <= phase_bar
        differ = got[..., n_pos:] != rows64[..., n_pos:]
        differ32 = rows32[..., n_pos:] != rows64[..., n_pos:]
        shares = (float(differ32.mean()), float(differ.mean()), int((differ & ~near).sum()))
        line += (f"; adhesion entries that differ: spec32-vs-spec64 {shares[0]:.3e}, kernel {shares[1]:.3e} (cap 1e-3), "
                 f"{shares[2]} of them away from a bin edge")
    print(line)
    return dict(row_err=row_err, row_bar=row_bar, phase_err=phase_err, phase_bar=phase_bar, mag_ulps=mag_ulps, shares=shares)


@pytest.mark.parametrize("preset, adhesion", [("legs_only", None), ("legs_only", ADHESION), ("all_possible", None),
                                              ("all_possible", ADHESION)])
def test_parity_with_the_specification(torch_mod, preset, adhesion):
    """67 worlds, perturbed start phases, 400 steps as launches of 1, 20, 37, 64, 64, 64, 64, 64, 22 with a new drive before each
    (zeros, ones and negative values among them), rows of 42 / 48 / 72 / 78 columns.  Against tests/cpg_spec.py in float64 on the same
    inputs: rows within max(4 x the largest |spec32 - spec64| on these inputs, 1.9e-6 rad = 4 ulp at 4 rad), the phases after
    every launch by the same rule in cycles, the magnitudes within 4 float32 ulp of their value; adhesion columns may differ only
    where the specification's phase lies within the phase bar of a bin edge, in at most 1e-3 of the entries.
    Measured: profiles/turning_cpg_parity.txt."""
    start, drives = _scenario()
    with _controller(preset, adhesion) as cpg:
        assert cpg.n_act == {"legs_only": 42, "all_possible": 72}[preset] + (6 if adhesion else 0)
        got, states = _run_gpu(torch_mod, cpg, start, drives, LAUNCHES)
        assert got.shape == (N, 400, cpg.n_act) and np.isfinite(got).all()
        fig = _compare(f"{preset} {cpg.n_act} columns", cpg, got, states, start, drives, LAUNCHES)
    assert fig["row_err"] <= fig["row_bar"], fig
    assert fig["phase_err"] <= fig["phase_bar"], fig
    assert fig["mag_ulps"] <= 4.0, fig
    if adhesion:
        assert set(np.unique(got[..., -6:])) <= set(ADHESION)
        assert fig["shares"][2] == 0 and fig["shares"][1] <= 1e-3, fig


def test_unit_drive_reproduces_the_tripod_table(torch_mod):
    """2500 steps of 67 freshly reset worlds under the unit drive against ``TripodCPG.targets(67, 2500, device=...)`` (with the
    adhesion columns): within the row bar of the parity test, computed for these inputs; adhesion entries differ in at most 1e-3."""
    torch = torch_mod
    launches = (64,) * 39 + (4,)
    start = spec.reset_phases(N)
    drives = np.ones((len(launches), N, 2), dtype=np.float32)
    with _controller("legs_only", ADHESION) as cpg:
        got, states = _run_gpu(torch, cpg, start, drives, launches)
        ref = cpg.targets(N, 2500, device=cpg.sim.device, adhesion=(cpg.stance,) + ADHESION).cpu().numpy()
        rows64, _ = _run_spec(cpg, start, drives[:1], (2500,), np.float64)
        rows32, _ = _run_spec(cpg, start, drives[:1], (2500,), np.float32)
        assert all(np.array_equal(m, np.ones_like(m)) for _, m in states)
    bar = max(4.0 * float(np.abs(rows32[..., :42].astype(np.float64) - rows64[..., :42]).max()), FLOOR)
    err = float(np.abs(got[..., :42].astype(np.float64) - ref[..., :42]).max())
    share = float((got[..., 42:] != ref[..., 42:]).mean())
    print(f"turning cpg, unit drive, 2500 steps against TripodCPG.targets: rows {err:.3e} rad (bar {bar:.3e}), "
          f"against the float64 specification {float(np.abs(got[..., :42] - rows64[..., :42]).max()):.3e}; adhesion entries that differ {share:.3e}")
    assert err <= bar and share <= 1e-3


def test_exact_continuity_and_batch_independence(torch_mod):
    """``advance(20)`` twice is bit for bit ``advance(40)``; world w of the 67-world controller equals, bitwise, world w - first of
    a 5-world controller placed at first / 67 with the same phases and drives (other lanes, other workgroup); ``advance(37)`` into
    a 64-step table leaves rows 37..63 and everything behind the table untouched."""
    torch = torch_mod
    start, drives = _scenario()
    with _controller(adhesion=ADHESION) as a, _controller(adhesion=ADHESION) as b:
        for c in (a, b):
            c.phase.copy_(torch.as_tensor(np.array(start), device=c.sim.device))
            c.set_drive(drives[0])
        first = a.advance(20)[:, :20].clone()
        second = a.advance(20)[:, :20].clone()
        whole = b.advance(40)[:, :40].clone()
        assert torch.equal(torch.cat([first, second], dim=1), whole) and not torch.equal(first, second)
        assert torch.equal(a.phase, b.phase) and torch.equal(a.magnitude, b.magnitude)
        # canary: a table inside a larger buffer
        size = N * 64 * a.n_act
        canvas = torch.full((size + 4096,), 1234.5, dtype=torch.float32, device=a.sim.device)
        a.table = canvas[:size].view(N, 64, a.n_act)
        out = a.advance(37)
        torch.cuda.synchronize()
        assert bool((out[:, 37:] == 1234.5).all()) and bool((canvas[size:] == 1234.5).all())
        assert bool((out[:, :37] != 1234.5).all())
    for first_world in (31, 62):                       # worlds 62..66 are the partly filled last workgroup of the big batch
        with _controller(adhesion=ADHESION) as big, _controller(adhesion=ADHESION, n=5) as small:
            big.reset()
            small.reset(first_world=first_world, total_worlds=N)
            torch.cuda.synchronize()
            assert torch.equal(small.phase, big.phase[first_world:first_world + 5])
            for k, n_steps in enumerate((20, 64, 5)):
                big.set_drive(drives[k])
                small.set_drive(drives[k][first_world:first_world + 5])
                rb, rs = big.advance(n_steps), small.advance(n_steps)
                assert torch.equal(rs[:, :n_steps], rb[first_world:first_world + 5, :n_steps]), (first_world, k)
            assert torch.equal(small.phase, big.phase[first_world:first_world + 5])
            assert torch.equal(small.magnitude, big.magnitude[first_world:first_world + 5])


def test_masked_reset(torch_mod):
    """After 300 steps with mixed drives ``reset(mask)`` makes half the worlds bit-equal to a freshly created controller and leaves
    the other half as it was."""
    torch = torch_mod
    _, drives = _scenario()
    with _controller() as cpg, _controller() as fresh:
        for k, n_steps in enumerate((64, 64, 64, 64, 44)):
            cpg.set_drive(drives[k])
            cpg.advance(n_steps)
        before = [v.clone() for v in (cpg.phase, cpg.magnitude, cpg.drive)]
        mask = torch.arange(N, device=cpg.sim.device) % 2 == 0
        cpg.reset(mask.cpu().numpy())
        torch.cuda.synchronize()
        for now, was, new in zip((cpg.phase, cpg.magnitude, cpg.drive), before, (fresh.phase, fresh.magnitude, fresh.drive)):
            assert torch.equal(now[mask], new[mask]) and torch.equal(now[~mask], was[~mask])
            assert not torch.equal(was[mask], new[mask])
        assert bool((fresh.drive == 1).all()) and bool((fresh.magnitude == 1).all())
        assert np.abs(fresh.phase.cpu().numpy() - spec.reset_phases(N)).max() < 1e-15


def test_one_control_tick_is_one_captured_graph(torch_mod):
    """A drive scatter + ``advance(20)`` + ``step_replay`` + ``pack_observations`` captured with ``torch.cuda.graph`` on the batch's
    stream (a single chain) replays, ten times with the drive changed in place, to state, table and observations bit-identical to
    the eager sequence: the controller's launch allocates nothing and never synchronises."""
    torch = torch_mod
    rng = np.random.default_rng(7)
    ticks = []
    for copy in (1, 2):
        cpg = _controller(adhesion=ADHESION, copy=copy)
        sim = cpg.sim
        obs = torch.zeros((N, 2 * (sim.model.nv - 6) + 42 + 96), dtype=torch.float32, device=sim.device)
        staged = torch.ones((N, 2), dtype=torch.float32, device=sim.device)
        rows = torch.arange(0, N, 2, device=sim.device)

        def tick(cpg=cpg, sim=sim, obs=obs, staged=staged, rows=rows):
            cpg.drive.index_copy_(0, rows, staged[rows])                # the scatter: every other world takes a new drive
            sim.step_replay(cpg.advance(20), cpg.act_ids, 0, 20)
            sim.pack_observations(obs)

        torch.zeros_like(cpg.drive).index_copy_(0, rows, staged[rows])      # (torch's own kernels are loaded before the capture)
        ticks.append((cpg, sim, obs, staged, tick))
    torch.cuda.synchronize()
    (c0, s0, o0, d0, eager), (c1, s1, o1, d1, captured) = ticks
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                              # captured before this controller has ever been advanced
        captured()
    tables = []
    for k in range(10):
        new = torch.as_tensor(rng.uniform(-0.5, 1.5, (N, 2)).astype(np.float32), device=s0.device)
        d0.copy_(new); d1.copy_(new)
        g.replay()
        eager()
        torch.cuda.synchronize()
        assert torch.equal(c0.table, c1.table) and torch.equal(c0.phase, c1.phase) and torch.equal(c0.magnitude, c1.magnitude), k
        assert torch.equal(c0.drive, c1.drive) and torch.equal(o0, o1), k
        for key in KEYS:
            assert torch.equal(s0.field(key), s1.field(key)), (k, key)
        tables.append(c0.table[:, :20].clone())
    assert not torch.equal(tables[0], tables[-1]) and bool(torch.isfinite(o0).all())
    assert bool((c0.drive[1::2] == 1).all()) and not bool((c0.drive[0::2] == 1).all())
    c0.close(); c1.close()


def test_the_engine_does_not_notice_the_controller(torch_mod):
    """``step_replay`` over the table ``advance`` wrote, and over a ``.clone()`` of it on another batch: every state field bitwise
    equal after 400 steps."""
    torch = torch_mod
    _, drives = _scenario()
    with _controller(adhesion=ADHESION, copy=3) as cpg:
        other, _ = _batch(copy=4)
        for k in range(20):
            cpg.set_drive(drives[k % len(drives)])
            table = cpg.advance(20)
            cpg.sim.step_replay(table, cpg.act_ids, 0, 20)
            other.step_replay(table.clone(), cpg.act_ids, 0, 20)
        torch.cuda.synchronize()
        for key in KEYS:
            assert torch.equal(cpg.sim.field(key), other.field(key)), key
        assert bool(torch.isfinite(cpg.sim.field("qpos")).all())


def _yaw(q):
    w, x, y, z = q[:, 3], q[:, 4], q[:, 5], q[:, 6]
    return np.arctan2(2 * (w * z + x * y), 1 - 2 * (y * y + z * z))


def test_the_drive_steers_the_flies(torch_mod):
    """48 worlds in three groups of 16 under drives (1, 0.4), (1, 1), (0.4, 1): settle, then 10 000 steps in 20-step ticks through
    ``TurningCPG.step``.  The group-mean yaw change is ordered as on the CPU oracle (the fly turns towards the weaker side); no
    world overflows its contacts or leaves the finite numbers.  Measured: -86.1 +- 1.3, -75.3 +- 2.0, +14.3 +- 1.7 degrees."""
    torch = torch_mod
    with _controller(n=48) as cpg:
        sim = cpg.sim
        drive = np.repeat(np.array([[1.0, 0.4], [1.0, 1.0], [0.4, 1.0]], dtype=np.float32), 16, axis=0)
        cpg.set_drive(drive)
        y0 = _yaw(sim.field("qpos").cpu().numpy().astype(np.float64))
        for _ in range(500):
            cpg.step(20)
        torch.cuda.synchronize()
        qpos, qvel = sim.field("qpos").cpu().numpy().astype(np.float64), sim.field("qvel").cpu().numpy()
        turn = np.degrees(spec.wrap((_yaw(qpos) - y0) / (2 * np.pi)) * 2 * np.pi).reshape(3, 16)
        for name, g in zip(("(1, 0.4)", "(1, 1)", "(0.4, 1)"), turn):
            print(f"turning cpg steering, drive {name}: yaw change mean {g.mean():+.1f} deg, spread (std) {g.std():.1f}, "
                  f"min {g.min():+.1f}, max {g.max():+.1f}")
        assert np.isfinite(qpos).all() and np.isfinite(qvel).all() and bool(torch.isfinite(cpg.phase).all())
        assert sim.overflow_steps() == 0
        means = turn.mean(axis=1)
        assert means[0] < means[1] < means[2], means


def test_refusals_come_before_anything_is_launched(torch_mod):
    torch = torch_mod
    from flygym_amd import _native
    from flygym_amd.controllers import TurningCPG

    sim, fly = _batch()
    cpg = TurningCPG(sim, fly.name)
    assert cpg.phase.dtype == torch.float64 and tuple(cpg.phase.shape) == (N, 6)
    assert cpg.magnitude.dtype == torch.float32 and tuple(cpg.magnitude.shape) == (N, 6) and tuple(cpg.drive.shape) == (N, 2)
    assert tuple(cpg.table.shape) == (N, 64, 42)
    for bad in (0, 65, -3):
        with pytest.raises(ValueError, match="n_steps"):
            cpg.advance(bad)
        with pytest.raises(ValueError, match="n_steps"):
            cpg.step(bad)
    for bad in (np.ones((N, 3)), np.ones((N - 1, 2)), np.ones(2)):
        with pytest.raises(ValueError, match="Expected a drive of shape"):
            cpg.set_drive(bad)
    with pytest.raises(ValueError, match="reset mask"):
        cpg.reset(np.ones(N + 1, dtype=bool))
    with pytest.raises(ValueError):
        cpg.reset(first_world=1)
    with pytest.raises(ValueError):
        TurningCPG(sim, "nosuchfly")
    with pytest.raises(ValueError):
        TurningCPG(sim, fly.name, table_steps=0)
    # the library's own validation (a binding that skips the Python checks)
    lib = _native.lib()
    table = cpg.table.data_ptr()
    for args, text in (((0, table, 64), b"n_steps"), ((65, table, 64), b"n_steps"), ((1, None, 64), b"null table"),
                       ((1, table, 32), b"tables of 64 steps")):
        assert lib.nmf_cpg_advance(cpg._h, args[0], args[1], args[2], None) != 0 and text in lib.nmf_last_error(), args
    cyc = np.ascontiguousarray(cpg.cycle, dtype=np.float32)
    legs = np.ascontiguousarray(cpg.leg_of_dof, dtype=np.int32)
    bad_legs = legs.copy(); bad_legs[7] = 6
    assert not lib.nmf_cpg_create(sim._batch_h, ctypes.byref(cpg._params), cyc.ctypes.data, bad_legs.ctypes.data, None)
    assert b"leg_of_col[7]" in lib.nmf_last_error()
    from flygym_amd.controllers import _CpgParams
    one_bin = _CpgParams.from_buffer_copy(cpg._params); one_bin.n_bins = 1
    assert not lib.nmf_cpg_create(sim._batch_h, ctypes.byref(one_bin), cyc.ctypes.data, legs.ctypes.data, None)
    assert b"n_bins" in lib.nmf_last_error()
    torch.cuda.synchronize()
    assert bool((cpg.table == 0).all())                    # none of the refused calls wrote a row
    with cpg:
        pass
    with pytest.raises(RuntimeError, match="closed"):
        cpg.advance(1)
    with pytest.raises(RuntimeError, match="closed"):
        cpg.set_drive(np.ones((N, 2)))
    with pytest.raises(RuntimeError, match="closed"):
        cpg.reset()
    cpg.close()                                            # closing twice is fine
