"""Tethered flies off their anchor (test helper, no test): the models, the states and the weld residual of
``test_tethered_cpu.py`` and ``test_tethered_gpu.py``.  The norms are those of ``tumbling_states.py``.

A ``TetheredWorld`` holds the root by six bilateral rows, the world-axis components (w; v) of the root twist, with the residual
``(2 sign(qe.w) vec(qe); pos - weld_pos)``, ``qe = q conj(weld_quat)``.  There is no ground, so no contact and no active set: the
constrained step is an unconstrained quadratic and can be held as tightly as free flight.  The worlds here spawn at a generic
attitude (world and body axes of the root differ, so a twist or a wrench taken in the wrong frame, or a ``weld_quat`` conjugated
the wrong way round, shows), and the states start the root *off* the anchor: by 0, 3e-6, 1e-5 (inside the impedance width of
1e-5), 1e-3 and 0.3 (mm along a random direction, rad about a random world axis), with velocities of 0 / 1 / 10 / 100 on every
dof, the root's included (the weld's damping term), and with the root quaternion of either sign (``sg``).

Every input is rounded to float32 before anyone sees it.  The spawn position is float32-representable, so that the small
residuals are the same numbers in float32 and in float64; the spawn quaternion is not (no generic unit quaternion of dyadic
rationals exists), which puts a residual of a few 1e-8 under every tier.

A sixth tier of 3.0 (rotation error near pi) is left out.  The residual's rotational part is the error quaternion's vector part,
``2 sin(delta / 2)``: 1.995 at 3.0 rad, so the tier could not be "what it says" to the 1 % that the large tiers are held to, and
five offsets crossed with four velocities and two signs already fill the 40 worlds.
"""

from __future__ import annotations

import numpy as np

from test_classify_check import CUSTOM_TREE, CUSTOM_TREE_LARGE
from tumbling_states import ACT_ADHESION, _f32, oracle_step

N_STATES = 41
OFFSETS = (0.0, 3e-6, 1e-5, 1e-3, 0.3)             # mm and rad; the weld's solimp width is 1e-5
VELOCITIES = (0.0, 1.0, 10.0, 100.0)
SPAWN_POS = (0.25, -0.5, 1.5)                      # float32-representable
SPAWN_QUAT = (0.5, -0.1, 0.7, 0.5)                 # unit (0.25 + 0.01 + 0.49 + 0.25), no axis of it is a world axis

# case -> (how the fly is built, create options, (kernel_family, terrain_kernel, tether_kernel)) as ``batch_info()`` reports them
CASES = {
    "legs_only": (("preset", "LEGS_ONLY"), {}, (0, 0, 1)),
    "legs_active_only": (("preset", "LEGS_ACTIVE_ONLY"), {}, (1, 0, 1)),
    "custom_tree": (("custom", CUSTOM_TREE), {}, (2, 0, 1)),
    "custom_tree_large": (("custom", CUSTOM_TREE_LARGE), {}, (3, 0, 1)),
    "all_biological": (("preset", "ALL_BIOLOGICAL"), {}, (4, 0, 1)),
    "all_biological-tables": (("preset", "ALL_BIOLOGICAL"), dict(rest_slow=True), (4, 0, 1)),
    "all_possible": (("preset", "ALL_POSSIBLE"), {}, (5, 0, 1)),
    "all_possible-tables": (("preset", "ALL_POSSIBLE"), dict(rest_slow=True), (5, 0, 1)),
}
CPU_CASES = [c for c in CASES if not c.endswith("-tables")]      # the options change the kernel's passes, not the model


def tethered_world(kind, arg, pos=SPAWN_POS, quat=SPAWN_QUAT):
    """A ``TetheredWorld`` with one fly: a preset's skeleton, or (``"custom"``) a preset's skeleton without the joints of the
    named parts; leg position actuators (kp 50) and leg adhesion."""
    import flygym_amd.compose as C
    from flygym_amd import anatomy as A
    from flygym_amd.utils.math import Rotation3D

    if kind == "preset":
        sk = A.Skeleton(axis_order=A.AxisOrder.YAW_PITCH_ROLL, joint_preset=getattr(A.JointPreset, arg))
    else:
        preset, drop = arg
        full = A.Skeleton(axis_order=A.AxisOrder.YAW_PITCH_ROLL, joint_preset=getattr(A.JointPreset, preset))
        keep = [j for j in full.anatomical_joints if not any(k in j.child.name for k in drop)]
        sk = A.Skeleton(axis_order=A.AxisOrder.YAW_PITCH_ROLL, anatomical_joints=keep)
    fly = C.Fly(name="t")
    fly.add_joints(sk, neutral_pose=C.KinematicPosePreset.NEUTRAL)
    legs = A.Skeleton(axis_order=A.AxisOrder.YAW_PITCH_ROLL, joint_preset=A.JointPreset.LEGS_ONLY)
    fly.add_actuators(legs.get_actuated_dofs_from_preset("legs_active_only"), C.ActuatorType.POSITION, kp=50.0,
                      neutral_input=C.KinematicPosePreset.NEUTRAL)
    fly.add_leg_adhesion()
    world = C.TetheredWorld()
    world.add_fly(fly, tuple(pos), Rotation3D("quat", tuple(quat)))
    return world


def family_model(name):
    """``(world, options, (kernel_family, terrain_kernel, tether_kernel))`` of one case; a fresh world on every call."""
    (kind, arg), options, info = CASES[name]
    return tethered_world(kind, arg), dict(options), info


def qmul(a, b):
    """Hamilton product of quaternions (w, x, y, z)."""
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def rotation(axis, angle):
    axis = np.asarray(axis, dtype=np.float64)
    return np.array([np.cos(0.5 * angle), *(np.sin(0.5 * angle) * axis / np.linalg.norm(axis))])


def anchor(model):
    """The weld's target pose as the compiler wrote it: ``(pos[3], quat[4])``."""
    p = np.asarray(model["weld_params"], dtype=np.float64)
    return p[0:3].copy(), p[3:7].copy()


def weld_residual(model, qpos):
    """``(res[6], qe[4])`` of one root pose, in float64, as the rows are stated: rotational part first."""
    pos, quat = anchor(model)
    q = np.asarray(qpos[3:7], dtype=np.float64)
    qe = qmul(q / np.linalg.norm(q), quat * np.array([1.0, -1.0, -1.0, -1.0]))
    sg = -2.0 if qe[0] < 0 else 2.0
    return np.concatenate([sg * qe[1:4], np.asarray(qpos[0:3], dtype=np.float64) - pos]), qe


def _recipe(w):
    return (3 if w == 40 else w) % 20


def offset_tier(w):
    return OFFSETS[_recipe(w) % 5]


def velocity_tier(w):
    return VELOCITIES[_recipe(w) // 5]


def negated(w):
    return 20 <= w < 40


def tier_worlds(delta, n=N_STATES):
    return [w for w in range(n) if offset_tier(w) == delta]


def states(model, seed):
    """41 states of ``model`` (a ``CompiledModel`` of a tethered world) as ``(qpos[41, nq], qvel[41, nv], ctrl[41, nu])``:
    float64 arrays of float32-representable values.  World w < 20: the root at the anchor composed with an offset of
    ``OFFSETS[w % 5]`` (that many mm along a random direction; that many rad about a random world axis, ``q = dq weld_quat``),
    velocities ``VELOCITIES[w // 5]`` on every dof, joint angles keyframe + N(0, 0.4), control noise on the odd worlds, adhesion
    on.  Worlds 20-39: the same recipe (fresh draws) with the root quaternion negated.  World 40 repeats world 3."""
    rng = np.random.default_rng(seed)
    nv, nu = model.nv, model.nu
    key_q, key_c = np.asarray(model["key_qpos"], dtype=np.float64), np.asarray(model["key_ctrl"], dtype=np.float64)
    adhesion = np.asarray(model["act_type"]) == ACT_ADHESION
    pos0, quat0 = anchor(model)
    qpos, qvel, ctrl = np.zeros((N_STATES, nv + 1)), np.zeros((N_STATES, nv)), np.zeros((N_STATES, nu))
    for w in range(N_STATES - 1):
        delta = offset_tier(w)
        direction, axis = rng.normal(size=3), rng.normal(size=3)
        qpos[w, 0:3] = pos0 + delta * direction / np.linalg.norm(direction)
        quat = qmul(rotation(axis, delta), quat0)
        qpos[w, 3:7] = -quat if negated(w) else quat
        qpos[w, 7:] = key_q[7:] + rng.normal(0, 0.4, nv - 6)
        qvel[w] = velocity_tier(w) * rng.normal(0, 1, nv)
        ctrl[w] = key_c
        if w % 2 == 1:
            ctrl[w, ~adhesion] += rng.normal(0, 0.25, int((~adhesion).sum()))
        ctrl[w, adhesion] = 1.0
    qpos[40], qvel[40], ctrl[40] = qpos[3], qvel[3], ctrl[3]
    return _f32(qpos), _f32(qvel), _f32(ctrl)


def step(o, qpos, qvel, ctrl, n=1, check_every=0):
    """``tumbling_states.oracle_step`` plus the last step's solver iterations."""
    out = oracle_step(o, qpos, qvel, ctrl, n, check_every)
    out["solver_iter"] = o.ints()["solver_iter"]
    return out


def tier_worst(dev, key, delta, n=N_STATES):
    """Worst of ``dev[w][key]`` over the worlds of one offset tier."""
    return max(dev[w][key] for w in tier_worlds(delta, n))


def residual_history(o, model, qpos, qvel, ctrl, n):
    """``|res|[n + 1, 6]``: the weld rows' residuals of oracle ``o`` at the given state and after each of ``n`` steps from it."""
    o.reset()
    o.qpos[:] = qpos; o.qvel[:] = qvel; o.ctrl[:] = ctrl
    o.arr("qacc_warmstart")[:] = 0
    hist = [weld_residual(model, o.qpos)[0]]
    for _ in range(n):
        o.step(1)
        hist.append(weld_residual(model, o.qpos)[0])
    return np.abs(np.array(hist))


def crossed_the_width(hist, width):
    """Whether some weld row was inside the impedance width at one step of the history and outside it at another."""
    inside = hist < width
    return bool((inside.any(axis=0) & (~inside).any(axis=0)).any())
