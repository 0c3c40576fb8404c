"""Tumbling flies in free flight (test helper, no test): the models, the states and the two norms of
``test_tumbling_cpu.py`` and ``test_tumbling_gpu.py``.

A fly 50 mm above the ground makes no contact at any attitude, so one step from such a state involves no solver, no active-set
history and no chaotic branch: ``qacc`` is the smooth pipeline alone (kinematics, inertias, bias, passive forces, actuation,
the articulated-body solve, the implicit-damping integrator) and can be held far tighter than a step in contact, in a norm
that weighs every dof by its inertia.  The states put the velocity terms in charge (up to |v| ~ 1000 on every dof, root
included), turn the root to any attitude and wrap every joint angle to +-40 rad, so that the half angles the kinematics pass
hands to ``sincos_bounded`` reach every quadrant with both signs.

Every input is rounded to float32 before anyone sees it: the kernel and both oracles start from identical numbers.
"""

from __future__ import annotations

import numpy as np

from test_classify_check import CUSTOM_TREE, CUSTOM_TREE_LARGE, custom_world

N_STATES = 41
TIERS = (0.0, 1.0, 10.0, 100.0, 1000.0)
ACT_ADHESION = 1                                   # flygym_amd/compiler/model.py

# case -> (how it is built, create options, kernel_family, terrain_kernel) as ``batch_info()`` reports them
CASES = {
    "legs_only": (("preset", "legs_only"), {}, 0, 0),
    "legs_active_only": (("preset", "legs_active_only"), {}, 1, 0),
    "custom_tree": (("custom", CUSTOM_TREE), {}, 2, 0),
    "custom_tree_large": (("custom", CUSTOM_TREE_LARGE), {}, 3, 0),
    "all_biological": (("preset", "all_biological"), {}, 4, 0),
    "all_biological-tables": (("preset", "all_biological"), dict(rest_slow=True), 4, 0),
    "all_possible": (("preset", "all_possible"), {}, 5, 0),
    "all_possible-tables": (("preset", "all_possible"), dict(rest_slow=True), 5, 0),
    "legs_only_on_blocks": (("terrain", ("LEGS_ONLY", "BlocksTerrainWorld")), {}, 0, 1),
    "all_biological_on_mixed": (("terrain", ("ALL_BIOLOGICAL", "MixedTerrainWorld")), {}, 4, 1),
}
CPU_CASES = [c for c in CASES if not c.endswith("-tables")]      # the options change the kernel's passes, not the model


def _terrain_world(preset, world_cls):
    """The preset's skeleton with the benchmark model's leg actuators and adhesion, and joint sites on the tibiae and the last
    tarsal segments, on a terrain of box cells (the ``Terrain<>`` kernel instantiations)."""
    import flygym_amd.compose as C
    from flygym_amd import anatomy as A
    from flygym_amd.utils.math import Rotation3D

    fly = C.Fly(name="t")
    sk = A.Skeleton(axis_order=A.AxisOrder.YAW_PITCH_ROLL, joint_preset=getattr(A.JointPreset, preset))
    fly.add_joints(sk, neutral_pose=C.KinematicPosePreset.NEUTRAL)
    legs = A.Skeleton(axis_order=A.AxisOrder.YAW_PITCH_ROLL, joint_preset=A.JointPreset.LEGS_ONLY)
    fly.add_actuators(legs.get_actuated_dofs_from_preset("legs_active_only"), C.ActuatorType.POSITION, kp=50.0,
                      neutral_input=C.KinematicPosePreset.NEUTRAL)
    fly.add_leg_adhesion()
    fly.add_joint_sites([j for j in sk.anatomical_joints if j.child.name.endswith(("tibia", "tarsus5"))])
    world = getattr(C, world_cls)()
    world.add_fly(fly, (0.3, 0.2, 0.8), Rotation3D("quat", (1, 0, 0, 0)))
    return world


def family_model(name):
    """``(world, options, (kernel_family, terrain_kernel))`` of one case; a fresh world on every call (``HIPSimulation``
    rewrites its world's noslip option in place)."""
    from flygym_amd import make_model

    (kind, arg), options, family, terrain = CASES[name]
    if kind == "preset":
        world = make_model(joints_preset=arg)[1]
    elif kind == "custom":
        world = custom_world(*arg)
    else:
        world = _terrain_world(*arg)
    return world, dict(options), (family, terrain)


def family_models():
    return {name: family_model(name) for name in CASES}


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def states(model, seed):
    """41 states of ``model`` (a ``CompiledModel``) as ``(qpos[41, nq], qvel[41, nv], ctrl[41, nu])``: float64 arrays of
    float32-representable values.  World w: velocity tier ``TIERS[w % 5]``; joint angles near the keyframe when ``w // 5`` is
    even, anywhere in +-40 rad when it is odd; control noise when ``w // 10`` is odd; world 40 repeats world 3."""
    rng = np.random.default_rng(seed)
    nv, nu = model.nv, model.nu
    key_q, key_c = np.asarray(model["key_qpos"], dtype=np.float64), np.asarray(model["key_ctrl"], dtype=np.float64)
    adhesion = np.asarray(model["act_type"]) == ACT_ADHESION
    qpos, qvel, ctrl = np.zeros((N_STATES, nv + 1)), np.zeros((N_STATES, nv)), np.zeros((N_STATES, nu))
    for w in range(N_STATES - 1):
        qpos[w, 0:3] = rng.normal(0, 1, 3) + np.array([0.0, 0.0, 50.0])
        quat = rng.normal(size=4)
        qpos[w, 3:7] = _f32(quat / np.linalg.norm(quat))
        if (w // 5) % 2 == 0:
            qpos[w, 7:] = key_q[7:] + rng.normal(0, 0.4, nv - 6)
        else:
            qpos[w, 7:] = rng.uniform(-40.0, 40.0, nv - 6)
        qvel[w] = TIERS[w % 5] * rng.normal(0, 1, nv)
        ctrl[w] = key_c
        if (w // 10) % 2 == 1:
            ctrl[w, ~adhesion] += rng.normal(0, 0.25, int((~adhesion).sum()))
        ctrl[w, adhesion] = 1.0
    qpos[40], qvel[40], ctrl[40] = qpos[3], qvel[3], ctrl[3]
    return _f32(qpos), _f32(qvel), _f32(ctrl)


def tier(w):
    return TIERS[(3 if w == 40 else w) % 5]


def narrow(w):
    return ((3 if w == 40 else w) // 5) % 2 == 0


def symmetrised(M_flat, nv):
    M = np.asarray(M_flat, dtype=np.float64).reshape(nv, nv)
    return np.tril(M) + np.tril(M, -1).T


def energy_norm(x, M):
    return float(np.sqrt(x @ M @ x))


def energy_err(e, a, M):
    """``sqrt(e'Me) / sqrt(a'Ma)``: the error's kinetic-energy norm relative to the acceleration's."""
    return energy_norm(e, M) / energy_norm(a, M)


def dof_err(e, a, M):
    """``max_j |e_j| / max(|a_j|, sqrt(a'Ma) / sqrt(M_jj))``: every dof relative to its own acceleration, or to the one that
    carries the whole acceleration's energy on that dof alone where its own is smaller."""
    return float((np.abs(e) / np.maximum(np.abs(a), energy_norm(a, M) / np.sqrt(np.diag(M)))).max())


def quat_err(q, ref):
    """Largest component difference of unit quaternions ``[n, 4]``, up to the sign of each."""
    q, ref = np.asarray(q, dtype=np.float64).reshape(-1, 4), np.asarray(ref, dtype=np.float64).reshape(-1, 4)
    return float(np.minimum(np.abs(q - ref).max(axis=1), np.abs(q + ref).max(axis=1)).max())


QUANTITIES = ("energy", "dof", "seg_xpos", "seg_xquat", "site_xpos", "actuator_force", "qvel_step", "qpos")


def deviations(got, ref, qvel0, h):
    """Every compared quantity of one step from one state: ``got`` against ``ref`` (dicts of the fields below; ``ref`` is the
    float64 oracle and brings ``M``).  ``qvel_step`` is the step's velocity change as an acceleration, ``(qvel1 - qvel0) / h``,
    in the energy norm: the implicit-damping solve on top of ``qacc``."""
    M = symmetrised(ref["M"], len(qvel0))
    e, a = got["qacc"] - ref["qacc"], ref["qacc"]
    out = dict(energy=energy_err(e, a, M), dof=dof_err(e, a, M),
               seg_xpos=float(np.abs(got["seg_xpos"] - ref["seg_xpos"]).max()),
               seg_xquat=quat_err(got["seg_xquat"], ref["seg_xquat"]),
               qvel_step=energy_err((got["qvel"] - ref["qvel"]) / h, (ref["qvel"] - qvel0) / h, M),
               qpos=float(np.abs(got["qpos"] - ref["qpos"]).max()))
    out["site_xpos"] = float(np.abs(got["site_xpos"] - ref["site_xpos"]).max()) if ref["site_xpos"].size else 0.0
    frc = ref["actuator_force"]
    out["actuator_force"] = float(np.abs(got["actuator_force"] - frc).max() / np.abs(frc).max()) if frc.size else 0.0
    return out


FIELDS = ("qacc", "qpos", "qvel", "seg_xpos", "seg_xquat", "site_xpos", "actuator_force", "M")


def oracle_step(o, qpos, qvel, ctrl, n=1, check_every=0):
    """Oracle ``o`` reset and stepped ``n`` times from the given state (warm start 0): its fields as float64 copies, the
    clock, and the largest contact count seen every ``check_every`` steps and at the end."""
    o.reset()
    o.qpos[:] = qpos; o.qvel[:] = qvel; o.ctrl[:] = ctrl
    o.arr("qacc_warmstart")[:] = 0
    ncon, left = 0, n
    while left > 0:
        k = min(left, check_every) if check_every else left
        o.step(k)
        left -= k
        ncon = max(ncon, o.ints()["ncon"])
    out = {k: np.array(o.arr(k), dtype=np.float64) for k in FIELDS}
    out["ncon"], out["time"] = ncon, o.time
    return out
