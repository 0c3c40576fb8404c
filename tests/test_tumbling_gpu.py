"""The HIP step kernel against the float64 oracle on tumbling flies in free flight, every kernel family (MI355X).

The states of ``tumbling_states.py``: 41 worlds 50 mm above the ground, root attitude uniform on the sphere, velocities of
0 / 1 / 10 / 100 / 1000 on every dof (root included), joint angles near the keyframe or anywhere in +-40 rad, control noise on
half of them.  No contact, so no solver and no chaotic branch: one step is the smooth pipeline in float32 and nothing else
— kinematics at random attitudes and wrapped angles (``sincos_bounded`` in every quadrant, both signs), inertias, the
velocity terms of the bias pass (0.88 to 0.999 of ``qacc`` in the fast tiers, a rounding-level share of it in every walking
state), actuation, the articulated-body solve and the implicit-damping integrator, on the unrolled leg chains, the tree
sweeps and both kinds of level passes (packed and ``rest_slow``'s tables).

``qacc`` is held in two norms that weigh a dof by its inertia (``energy_err``, ``dof_err``): the thorax's accelerations are
2e-3 to 2e-2 of the largest ``|qacc|`` (a tarsal hinge's), so the max-norm bars of the walking-state tests let a 10 % error
of them through; ``test_tumbling_cpu.py`` shows a 2 % error of the thorax's inertia missing the bars below on every tier.

**Bars**: every quantity 8 x the float32 oracle's deviation from the float64 oracle for the same quantity, worst over the case's
states, computed here from the two oracles and never from the kernel.  Why 8: the kernel is a different float32 algorithm
from the float32 oracle (articulated-body sweeps with ``v_rcp_f32`` pivots, DPP and LDS summation orders, a polynomial sincos
— against CRBA, LDL' and libm); their errors are of the same order, not equal.  ``test_tumbling_cpu.py`` caps the floors, so
a bar is at most 1.6e-4 (energy) / 8e-4 (per dof); the 2 % inertia error still exceeds those sixfold.

Kernel over float32 floor (1 = as accurate as the float32 oracle, the bar is 8), one MI355X, the commit that added the test:

    case                      energy   dof  seg_xpos seg_xquat site_xpos act_force qvel_step  qpos  50 steps: qpos  qvel
    legs_only                   1.67  0.51      1.86      3.61         -      0.56      0.60  0.99            0.86  1.18
    legs_active_only            1.30  1.60      2.07      2.37         -      0.70      0.82  1.01            1.00  1.18
    custom_tree                 1.77  0.74      1.47      3.00         -      0.76      0.57  1.02            1.00  0.79
    custom_tree_large           0.98  0.43      1.59      2.19         -      0.62      0.65  1.00            0.52  0.73
    all_biological              0.94  0.42      1.81      2.60         -      0.62      0.84  1.00            0.83  1.16
    all_biological-tables       0.94  0.42      1.81      2.60         -      0.62      0.84  1.00            0.83  1.16
    all_possible                1.01  1.17      2.16      2.38         -      0.68      0.73  0.95            1.39  1.36
    all_possible-tables         1.01  1.17      2.16      2.38         -      0.68      0.73  0.95            1.39  1.36
    legs_only_on_blocks         1.67  0.51      1.86      3.61      1.86      0.56      0.60  0.99            0.86  1.09
    all_biological_on_mixed     0.94  0.42      1.81      2.60      1.81      0.62      0.84  1.00            0.83  1.16

No quantity of any family is beyond 3.7 x the float32 oracle's own error (the largest: body quaternions, 7e-7
absolute); no defect of the kernel was found.  The table-driven level passes give the packed
ones' figures to every digit, as ``rest_slow`` promises.  Every run reports its figures through ``ledger.report``.
"""

import numpy as np
import pytest

import tumbling_states as T
from ledger import report

pytestmark = pytest.mark.gpu

SEED = 20                       # the states of test_tumbling_cpu.py
MARGIN = 8.0
ROLLOUT_STEPS, ROLLOUT_WORLDS = 50, 10
STEP_FIELDS = ("qacc", "qpos", "qvel", "seg_xpos", "seg_xquat", "site_xpos", "actuator_force")


def _push(sim, torch, qpos, qvel, ctrl):
    for name, a in (("qpos", qpos), ("qvel", qvel), ("ctrl", ctrl), ("qacc_warmstart", np.zeros_like(qvel))):
        sim.field(name)[:len(a)] = torch.as_tensor(a, dtype=torch.float32, device=sim.device)


@pytest.mark.parametrize("name", T.CASES)
def test_free_flight_step_and_rollout_against_float64(oracle_lib, name):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from flygym_amd import HIPSimulation

    world, options, family = T.family_model(name)
    n = T.N_STATES
    sim = HIPSimulation(world, n_worlds=n, device=0, _options=options)
    info = sim.batch_info()
    assert (info["kernel_family"], info["terrain_kernel"]) == family
    model, h = sim.model, sim.timestep
    blob = model.to_blob()
    o64, o32 = oracle_lib.Oracle(blob, "f64"), oracle_lib.Oracle(blob, "f32")
    qpos, qvel, ctrl = T.states(model, SEED)

    # ---- one step from each of the 41 states
    _push(sim, torch, qpos, qvel, ctrl)
    sim.step(1)
    torch.cuda.synchronize()
    got = {k: sim.field(k).cpu().numpy() for k in STEP_FIELDS}
    stats = sim.field("stats").cpu().numpy()
    assert np.all(stats[:, 0] == 0), stats[:, 0]                       # no contact in the kernel either, at any attitude
    floor = dict.fromkeys(T.QUANTITIES, 0.0)
    worst = dict.fromkeys(T.QUANTITIES, 0.0)
    where = dict.fromkeys(T.QUANTITIES, -1)
    for w in range(n):
        ref = T.oracle_step(o64, qpos[w], qvel[w], ctrl[w])
        f32 = T.oracle_step(o32, qpos[w], qvel[w], ctrl[w])
        assert ref["ncon"] == 0 and f32["ncon"] == 0
        dev_f = T.deviations(f32, ref, qvel[w], h)
        dev_k = T.deviations({k: got[k][w].astype(np.float64) for k in STEP_FIELDS}, ref, qvel[w], h)
        for k in T.QUANTITIES:
            floor[k] = max(floor[k], dev_f[k])
            if dev_k[k] > worst[k]:
                worst[k], where[k] = dev_k[k], w
    assert model.nsite == 0 or floor["site_xpos"] > 0                  # the terrain cases carry sites
    for k in STEP_FIELDS:                                              # world 40 repeats world 3: the same bits
        assert np.array_equal(got[k][40], got[k][3]), k

    # ---- 50 steps in one launch from the first ten states (the other worlds drop from the keyframe)
    sim.reset()
    _push(sim, torch, qpos[:ROLLOUT_WORLDS], qvel[:ROLLOUT_WORLDS], ctrl[:ROLLOUT_WORLDS])
    sim.step(ROLLOUT_STEPS)
    torch.cuda.synchronize()
    q_k, v_k = sim.field("qpos").cpu().numpy().astype(np.float64), sim.field("qvel").cpu().numpy().astype(np.float64)
    time_k = sim.field("time").cpu().numpy().astype(np.float64).reshape(-1)
    for k in ("rollout_qpos", "rollout_qvel"):
        floor[k], worst[k], where[k] = 0.0, 0.0, -1
    for w in range(ROLLOUT_WORLDS):
        r64 = T.oracle_step(o64, qpos[w], qvel[w], ctrl[w], ROLLOUT_STEPS, check_every=10)
        r32 = T.oracle_step(o32, qpos[w], qvel[w], ctrl[w], ROLLOUT_STEPS, check_every=10)
        assert r64["ncon"] == 0 and r32["ncon"] == 0
        vscale = max(1.0, np.abs(r64["qvel"]).max())
        for k, f, g in (("rollout_qpos", np.abs(r32["qpos"] - r64["qpos"]).max(), np.abs(q_k[w] - r64["qpos"]).max()),
                        ("rollout_qvel", np.abs(r32["qvel"] - r64["qvel"]).max() / vscale, np.abs(v_k[w] - r64["qvel"]).max() / vscale)):
            floor[k] = max(floor[k], float(f))
            if g > worst[k]:
                worst[k], where[k] = float(g), w
    # the clock: 50 float32 additions of h, each rounded to at most half a unit in the last place of the sum, and h's own rounding
    t_end = ROLLOUT_STEPS * h
    time_bar = ROLLOUT_STEPS * (0.5 * float(np.spacing(np.float32(t_end))) + abs(float(np.float32(h)) - h))
    time_err = float(np.abs(time_k - t_end).max())

    ratio = {k: (worst[k] / floor[k] if floor[k] > 0 else (0.0 if worst[k] == 0 else float("inf"))) for k in floor}
    report("test_tumbling_gpu", case=name, family=family[0], terrain=family[1], margin=MARGIN,
           floor=floor, kernel=worst, ratio={k: round(v, 3) for k, v in ratio.items()}, world=where,
           time_err=time_err, time_bar=time_bar)
    for k in floor:
        print(f"{name:24s} {k:15s} float32 floor {floor[k]:.3e}  kernel {worst[k]:.3e} (world {where[k]})  ratio {ratio[k]:.2f}")
    assert time_err <= time_bar, (time_err, time_bar)
    over = {k: (worst[k], MARGIN * floor[k], where[k]) for k in floor if worst[k] > MARGIN * floor[k]}
    assert not over, f"{name}: beyond {MARGIN:g} x the float32 oracle's deviation (kernel, bar, world): {over}"
