"""What float32 costs the smooth pipeline on tumbling flies, and what the energy norm sees (no GPU).

``test_tumbling_gpu.py`` holds the HIP kernel to 8 x the float32 oracle's deviation from the float64 oracle on the states of
``tumbling_states.py``.  This file keeps that bar honest without a GPU:

* the floors themselves stay under caps (about twice what was measured when the tests were written), so a bar derived from a
  floor cannot grow unnoticed; no state touches the ground in either oracle;
* the velocity terms really are the signal in the fast tiers;
* 50-step rollouts of the two oracles stay together;
* a float64 oracle of a model with the thorax's inertia 2 % off, or the inertia of a light body 5 % off, misses the new bar
  on every velocity tier and passes the old max-norm bar ``2e-3 * max(|qacc|.max(), 1e4)``: the written proof that the new
  test sees what the old bars let through.
"""

import functools

import numpy as np
import pytest

import tumbling_states as T

SEED = 20
CAPS = dict(energy=2e-5, dof=1e-4, seg_xpos=3e-5, seg_xquat=1e-6)


@functools.lru_cache(maxsize=None)
def _case(name):
    """The case's compiled model, its states, and every state stepped once on both oracles."""
    import oracle as orc

    orc.build()
    model = T.family_model(name)[0].compile_model()
    blob = model.to_blob()
    o64, o32 = orc.Oracle(blob, "f64"), orc.Oracle(blob, "f32")
    qpos, qvel, ctrl = T.states(model, SEED)
    ref = [T.oracle_step(o64, qpos[w], qvel[w], ctrl[w]) for w in range(T.N_STATES)]
    f32 = [T.oracle_step(o32, qpos[w], qvel[w], ctrl[w]) for w in range(T.N_STATES)]
    h = float(model["opt_timestep"][0])
    dev = [T.deviations(f32[w], ref[w], qvel[w], h) for w in range(T.N_STATES)]
    return dict(model=model, o64=o64, o32=o32, states=(qpos, qvel, ctrl), ref=ref, f32=f32, dev=dev, h=h)


def _worst(dev, key, worlds=range(T.N_STATES)):
    return max(dev[w][key] for w in worlds)


@pytest.mark.parametrize("name", T.CPU_CASES)
def test_float32_floors_stay_under_their_caps(name):
    c = _case(name)
    floors = {k: _worst(c["dev"], k) for k in T.QUANTITIES}
    print(name, "float32 oracle against float64 oracle, worst of 41 states:", {k: f"{v:.2e}" for k, v in floors.items()})
    assert max(r["ncon"] for r in c["ref"]) == 0 and max(r["ncon"] for r in c["f32"]) == 0
    for k, cap in CAPS.items():
        assert floors[k] <= cap, (k, floors[k], cap)
    qpos, qvel, ctrl = c["states"]
    for a in (qpos, qvel, ctrl):                                # what the kernel is given is what the oracles were given
        assert np.array_equal(a, a.astype(np.float32).astype(np.float64))
    assert np.array_equal(qpos[40], qpos[3]) and np.array_equal(qvel[40], qvel[3]) and np.array_equal(ctrl[40], ctrl[3])
    half = 0.5 * qpos[:, 7:][[w for w in range(40) if not T.narrow(w)]]
    assert half.min() < -19 and half.max() > 19                 # half angles over sincos_bounded's stated range,
    assert set(np.unique(np.rint(half / (np.pi / 2)).astype(int) & 3)) == {0, 1, 2, 3}    # in every quadrant


@pytest.mark.parametrize("name", T.CPU_CASES)
def test_velocity_terms_are_the_signal(name):
    """Share of the velocity terms in ``qacc``, ``|a(v) - a(v=0)|_M / |a(v)|_M``, on the narrow-angle states."""
    c = _case(name)
    qpos, qvel, ctrl = c["states"]
    shares = {100.0: [], 1000.0: []}
    for w in range(40):
        if T.narrow(w) and T.tier(w) in shares:
            a = c["ref"][w]["qacc"]
            a0 = T.oracle_step(c["o64"], qpos[w], 0 * qvel[w], ctrl[w])["qacc"]
            M = T.symmetrised(c["ref"][w]["M"], len(a))
            shares[T.tier(w)].append(T.energy_err(a - a0, a, M))
    print(name, "velocity share:", {k: f"min {min(v):.3f} of {len(v)}" for k, v in shares.items()})
    assert len(shares[100.0]) == len(shares[1000.0]) == 4
    assert min(shares[100.0]) >= 0.5 and min(shares[1000.0]) >= 0.9


ROLLOUT_STEPS = 50


@pytest.mark.parametrize("name", T.CPU_CASES)
def test_rollout_floors(name):
    c = _case(name)
    qpos, qvel, ctrl = c["states"]
    worst_q = worst_v = 0.0
    for w in range(10):
        r64 = T.oracle_step(c["o64"], qpos[w], qvel[w], ctrl[w], ROLLOUT_STEPS, check_every=10)
        r32 = T.oracle_step(c["o32"], qpos[w], qvel[w], ctrl[w], ROLLOUT_STEPS, check_every=10)
        assert r64["ncon"] == 0 and r32["ncon"] == 0
        dq = np.abs(r32["qpos"] - r64["qpos"]).max()
        dv = np.abs(r32["qvel"] - r64["qvel"]).max() / max(1.0, np.abs(r64["qvel"]).max())
        print(name, f"world {w}: qpos {dq:.2e} qvel {dv:.2e}")
        worst_q, worst_v = max(worst_q, dq), max(worst_v, dv)
    assert worst_q <= 1e-4 and worst_v <= 5e-5, (worst_q, worst_v)


def _changed(model, body, factor):
    out = type(model)({k: np.array(v) for k, v in model.items()})
    out.meta = dict(model.meta)
    out["body_inertia"][body] *= factor
    return out


@pytest.mark.parametrize("name", ["legs_only", "all_biological"])
@pytest.mark.parametrize("body,factor,metrics", [(0, 1.02, ("energy", "dof")), (3, 1.05, ("energy",))])
def test_a_wrong_inertia_misses_the_new_bar_and_passes_the_old(name, body, factor, metrics):
    import oracle as orc

    c = _case(name)
    qpos, qvel, ctrl = c["states"]
    wrong = orc.Oracle(_changed(c["model"], body, factor).to_blob(), "f64")
    dev, old = [], []
    for w in range(40):
        got = T.oracle_step(wrong, qpos[w], qvel[w], ctrl[w])
        dev.append(T.deviations(got, c["ref"][w], qvel[w], c["h"]))
        a = c["ref"][w]["qacc"]
        old.append(np.abs(got["qacc"] - a).max() / (2e-3 * max(np.abs(a).max(), 1e4)))
    passes = float(np.mean(np.array(old) < 1.0))
    if body == 0:                                                 # the max-norm bar of the walking-state tests lets it through
        assert max(old) < 1.0, max(old)
    else:                                                         # ... and most states of a light body's error, whose dofs
        assert passes > 0.5, (passes, max(old))                   # carry the largest accelerations themselves
    for k in metrics:
        bar = 8 * _worst(c["dev"], k)
        per_tier = {t: max(dev[w][k] for w in range(40) if T.tier(w) == t) for t in T.TIERS}
        print(name, f"body {body} inertia x {factor}: {k} per tier", {t: f"{v:.2e}" for t, v in per_tier.items()},
              f"bar {bar:.2e}, old bar used up to {max(old):.2f}, {passes:.0%} of the states pass it")
        assert min(per_tier.values()) > bar, (k, per_tier, bar)
