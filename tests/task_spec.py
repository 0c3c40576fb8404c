"""The walking task's specification in numpy (the kernel is ``flygym_amd/csrc/nmf_task.hip``, the class
``flygym_amd.tasks.WalkingTask``, the statement of the rule ``include/nmf.h``, ``nmf_task_update``).

Written from the definition, one update at a time, every world at once.  Everything is float32 and every operation is rounded on its
own; tests and clamps are comparisons (``np.where``), so a NaN fails them as in the kernel; counters are int32 that wrap; a stored
float that is a zero is +0.  Per world::

    bad      = an input has all exponent bits set            -> reason NONFINITE alone, reward -penalty_fail, a row of zeros
    progress = fresh ? 0 : (x - px) * cx + (y - py) * cy
    up_z     = 1 - 2 * (qx * qx + qy * qy);  tilt_count = up_z < cos_max_tilt ? tilt_count + 1 : 0
    flag_l   = found_l > 0 and (Fx * Fx + Fy * Fy) + Fz * Fz > thr2[l];  airborne_count = no flag ? airborne_count + 1 : 0
    P        = sum_a int32(rint(clamp(|f_a * qd_a|, 0, power_clip) * 2^10))  (0 for a term that is not finite);  power = float32(P) * 2^-10
    n = ep_length + 1;  grace = n <= grace_ticks;  reason bits TILTED, AIRBORNE, HEIGHT (none of them in grace), OUT_OF_ARENA, GOAL
    terminated = reason != 0;  truncated = not terminated and n >= max_ticks;  done = terminated or truncated
    r = alive;  r += w_progress * progress;  r -= w_power * power;  r -= w_tilt * (1 - up_z);  GOAL: r += bonus_goal;  other bit: r -= penalty_fail
    ep_return += r;  ep_length = n;  done: latch last_*, episodes += 1, successes += GOAL, start values;  else prev_xy = (x, y), fresh = 0
    obs = [-r20, -r21, -r22,  R^T v,  omega,  (R^T (goal - pos, 0))[:2],  z,  flags,  (ang - mean) * inv_std]

The second half of the module is the input generator and the settings the GPU parity tests use; ``tests/test_task_cpu.py`` asserts on
the specification alone that they reach every reason, truncation, the grace period and both kinds of counter run.
"""
import functools
from dataclasses import dataclass

import numpy as np

NONFINITE, TILTED, AIRBORNE, HEIGHT, OUT_OF_ARENA, GOAL = 1, 2, 4, 8, 16, 32
REASONS = dict(nonfinite=NONFINITE, tilted=TILTED, airborne=AIRBORNE, height=HEIGHT, out_of_arena=OUT_OF_ARENA, goal=GOAL)
POWER_BITS = 10
OBS_BODY = 12
# name -> (dtype, row width; None: 12 + 6 + n_q), in the order of the NMF_TASK_ field indices of include/nmf.h
LAYOUT = dict(reward=("f4", 1), obs=("f4", None), ep_return=("f4", 1), last_return=("f4", 1), prev_xy=("f4", 2), course=("f4", 2),
              goal=("f4", 2), terminated=("u1", 1), truncated=("u1", 1), done=("u1", 1), fresh=("u1", 1), reason=("i4", 1),
              ep_length=("i4", 1), last_length=("i4", 1), last_reason=("i4", 1), tilt_count=("i4", 1), airborne_count=("i4", 1),
              episodes=("i4", 1), successes=("i4", 1))
FIELDS = tuple(LAYOUT)
f32 = np.float32


@dataclass(frozen=True)
class Params:
    """``nmf_task_params`` without the indices and counts: float32 values, the tick counts ints."""

    tilt_ticks: int
    airborne_ticks: int
    max_ticks: int
    grace_ticks: int
    cos_max_tilt: float
    z_min: float
    z_max: float
    arena: tuple
    goal_radius2: float
    power_clip: float
    thr2: tuple
    alive: float = 0.0
    w_progress: float = 1.0
    w_power: float = 0.0
    w_tilt: float = 0.0
    bonus_goal: float = 0.0
    penalty_fail: float = 0.0

    def __post_init__(self):
        for name, value in list(self.__dict__.items()):
            if name.endswith("_ticks"):
                value = int(value)
            elif isinstance(value, (tuple, list)):
                value = tuple(f32(v) for v in value)
            else:
                value = f32(value)
            object.__setattr__(self, name, value)

    @classmethod
    def from_struct(cls, p):
        """From the ctypes mirror ``flygym_amd.tasks._TaskParams`` of a live task."""
        return cls(**{k: (tuple(getattr(p, k)) if k in ("arena", "thr2") else getattr(p, k)) for k in cls.__dataclass_fields__})


def odd(a):
    """All exponent bits set: NaN, +Inf, -Inf — on the bits."""
    return (np.ascontiguousarray(a, dtype=f32).view(np.uint32) & np.uint32(0x7F800000)) == np.uint32(0x7F800000)


def plus_zero(a):
    return np.where(a == 0, f32(0), a).astype(f32)


def power_sum(force, qd, power_clip):
    """``(P int32 (n,), power float32 (n,))`` of ``force``, ``qd`` ``(n, n_act)``."""
    with np.errstate(all="ignore"):
        m = np.abs(force * qd)
        c = np.where(m < 0, f32(0), np.where(m > power_clip, f32(power_clip), m)).astype(f32)
        scaled = np.where(odd(force) | odd(qd), f32(0), c * f32(2 ** POWER_BITS)).astype(f32)
        P = np.rint(scaled).astype(np.int32).sum(axis=1, dtype=np.int32)
    return P, P.astype(f32) * f32(2.0 ** -POWER_BITS)


class State:
    """The arrays of ``n`` worlds; ``mean`` / ``inv_std`` ``(n_q,)`` float32.  After an update ``last`` holds, per world, ``bad``,
    ``grace``, ``raw`` (the reason bits before the grace period took TILTED, AIRBORNE and HEIGHT away) and ``progress``."""

    def __init__(self, n, params, n_q, mean=None, inv_std=None):
        self.n, self.p, self.n_q = int(n), params, int(n_q)
        self.mean = np.zeros(n_q, dtype=f32) if mean is None else np.asarray(mean, dtype=f32)
        self.inv_std = np.ones(n_q, dtype=f32) if inv_std is None else np.asarray(inv_std, dtype=f32)
        for name, (dtype, width) in LAYOUT.items():
            width = OBS_BODY + 6 + self.n_q if width is None else width
            setattr(self, name, np.zeros((n, width) if width > 1 else n, dtype=np.dtype(dtype)))
        self.course[:, 0] = 1
        self.last = {}
        self.reset()

    def reset(self, mask=None):
        m = np.ones(self.n, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
        for name in FIELDS:
            if name not in ("course", "goal"):
                getattr(self, name)[m] = 0
        self.fresh[m] = 1

    def update(self, pos, quat, vel, force, qd, sens, ang):
        """``pos`` ``(n, 3)``, ``quat`` ``(n, 4)`` (w, x, y, z), ``vel`` ``(n, 6)`` (qvel[0:6]), ``force`` and ``qd`` ``(n, n_act)``,
        ``sens`` ``(n, 6, 4)`` (found, Fx, Fy, Fz per leg), ``ang`` ``(n, n_q)``."""
        p, n = self.p, self.n
        pos, quat, vel, force, qd, ang = (np.asarray(a, dtype=f32).reshape(n, -1) for a in (pos, quat, vel, force, qd, ang))
        sens = np.asarray(sens, dtype=f32).reshape(n, 6, 4)
        x, y, z = pos.T
        qw, qx, qy, qz = quat.T
        vx, vy, vz, ox, oy, oz = vel.T
        cx, cy = self.course.T
        gx, gy = self.goal.T
        one, two = f32(1), f32(2)
        bad = np.zeros(n, dtype=bool)
        for a in (pos, quat, vel, force, qd, sens.reshape(n, -1), ang, self.course, self.goal):
            bad |= odd(a).any(axis=1)
        with np.errstate(all="ignore"):
            fresh = self.fresh != 0
            progress = np.where(fresh, f32(0), (x - self.prev_xy[:, 0]) * cx + (y - self.prev_xy[:, 1]) * cy).astype(f32)
            up_z = one - two * (qx * qx + qy * qy)
            tilt = np.where(up_z < p.cos_max_tilt, self.tilt_count + np.int32(1), 0).astype(np.int32)
            f2 = (sens[:, :, 1] * sens[:, :, 1] + sens[:, :, 2] * sens[:, :, 2]) + sens[:, :, 3] * sens[:, :, 3]
            flags = (sens[:, :, 0] > 0) & (f2 > np.array(p.thr2, dtype=f32))
            air = np.where(~flags.any(axis=1), self.airborne_count + np.int32(1), 0).astype(np.int32)
            _, power = power_sum(force, qd, p.power_clip)
            length = self.ep_length + np.int32(1)
            grace = length <= p.grace_ticks
            dx, dy = gx - x, gy - y
            raw = (np.where(tilt >= p.tilt_ticks, TILTED, 0) | np.where(air >= p.airborne_ticks, AIRBORNE, 0)
                   | np.where((z < p.z_min) | (z > p.z_max), HEIGHT, 0)
                   | np.where((x < p.arena[0]) | (x > p.arena[1]) | (y < p.arena[2]) | (y > p.arena[3]), OUT_OF_ARENA, 0)
                   | np.where(dx * dx + dy * dy < p.goal_radius2, GOAL, 0))
            reason = np.where(grace, raw & ~(TILTED | AIRBORNE | HEIGHT), raw)
            reason = np.where(bad, NONFINITE, reason).astype(np.int32)
            terminated = reason != 0
            truncated = ~terminated & (length >= p.max_ticks)
            done = terminated | truncated

            r = np.full(n, p.alive, dtype=f32)
            r = r + p.w_progress * progress
            r = r - p.w_power * power
            r = r - p.w_tilt * (one - up_z)
            r = np.where(reason & GOAL, r + p.bonus_goal, r)
            r = np.where(reason & ~GOAL, r - p.penalty_fail, r)
            r = plus_zero(np.where(bad, -p.penalty_fail, r))
            ret = plus_zero(self.ep_return + r)

            r00, r01, r02 = one - two * (qy * qy + qz * qz), two * (qx * qy - qw * qz), two * (qx * qz + qw * qy)
            r10, r11, r12 = two * (qx * qy + qw * qz), one - two * (qx * qx + qz * qz), two * (qy * qz - qw * qx)
            r20, r21, r22 = two * (qx * qz - qw * qy), two * (qy * qz + qw * qx), up_z
            body = [-r20, -r21, -r22, (r00 * vx + r10 * vy) + r20 * vz, (r01 * vx + r11 * vy) + r21 * vz, (r02 * vx + r12 * vy) + r22 * vz,
                    ox, oy, oz, r00 * dx + r10 * dy, r01 * dx + r11 * dy, z]
            obs = np.concatenate([np.stack(body, axis=1), flags.astype(f32), (ang - self.mean) * self.inv_std], axis=1)
            assert obs.dtype == f32 and r.dtype == f32 and ret.dtype == f32 and power.dtype == f32 and progress.dtype == f32
            obs = np.where(bad[:, None], f32(0), plus_zero(obs)).astype(f32)

        self.reward, self.obs = r, obs
        self.terminated, self.truncated, self.done = (a.astype(np.uint8) for a in (terminated, truncated, done))
        self.reason = reason
        self.last_return = np.where(done, ret, self.last_return).astype(f32)
        self.last_length = np.where(done, length, self.last_length).astype(np.int32)
        self.last_reason = np.where(done, reason, self.last_reason).astype(np.int32)
        self.episodes = (self.episodes + done).astype(np.int32)
        self.successes = (self.successes + (done & ((reason & GOAL) != 0))).astype(np.int32)
        self.ep_return = np.where(done, f32(0), ret).astype(f32)
        self.ep_length = np.where(done, 0, length).astype(np.int32)
        self.tilt_count = np.where(done, 0, tilt).astype(np.int32)
        self.airborne_count = np.where(done, 0, air).astype(np.int32)
        self.fresh = done.astype(np.uint8)
        self.prev_xy = np.where(done[:, None], f32(0), np.stack([x, y], axis=1)).astype(f32)
        self.last = dict(bad=bad, grace=grace, raw=np.where(bad, NONFINITE, raw), progress=progress, tilt=tilt, air=air, was_fresh=fresh)

    def snapshot(self):
        return {name: np.copy(getattr(self, name)) for name in FIELDS}


# ---- what the GPU parity tests run: settings, inputs, reference runs -------------------------------------------------------

# 16 lanes per world, 4 worlds per wave, 16 per workgroup: one world, one past a wave's worth, one past a workgroup's worth, 257
CASES = ((1, 120), (5, 100), (17, 80), (257, 60))
COMBOS = ((1, 1), (17, 3), (42, 42))      # (n_act, n_q): one lane of a group busy, one past a group, the default
SEED = 33
PARITY = Params(tilt_ticks=3, airborne_ticks=4, max_ticks=12, grace_ticks=2, cos_max_tilt=0.5, z_min=0.5, z_max=2.5,
                arena=(-10.0, 10.0, -10.0, 10.0), goal_radius2=1.0, power_clip=50.0, thr2=(0.25, 1.0, 9.0, 0.25, 1.0, 9.0), alive=0.1,
                w_progress=2.0, w_power=0.01, w_tilt=0.5, bonus_goal=10.0, penalty_fail=5.0)
INPUTS = ("pos", "quat", "vel", "force", "qd", "sens", "ang")
_KINDS = np.array([np.nan, np.inf, -np.inf, 1e-40, -3e-42], dtype=f32)     # what is planted: three odd values, two denormals
_LAST_GOAL = (3.0, -2.0)


def standardisation(n_q):
    """``(mean, inv_std)`` ``(n_q,)`` float32 of the parity runs."""
    k = np.arange(n_q)
    return (0.1 * np.cos(k)).astype(f32), (1.0 / (0.5 + 0.1 * (k % 5))).astype(f32)


def _script():
    """The last world's ticks, 31 to a cycle whatever the inputs of the other worlds: an episode that runs into the time limit with
    a tilt run and an airborne run cut short, then one ended by each reason — HEIGHT after the grace period suppressed it once."""
    calm = dict(tilt=False, air=False, z="ok", out=False, goal=False, bad=False)
    t = lambda **kw: {**calm, **kw}
    a = [t() for _ in range(12)]
    a[3], a[4] = t(tilt=True), t(tilt=True)
    a[6], a[7], a[8] = t(air=True), t(air=True), t(air=True)
    b = [t(tilt=True)] * 3
    c = [t(z="low"), t(), t(), t(z="high")]
    d = [t(air=True)] * 4
    e = [t(), t(), t(out=True)]
    f = [t(), t(), t(goal=True)]
    g = [t(), t(bad=True)]
    return a + b + c + d + e + f + g


def _world(rng, T, n_act, n_q, goal, script=None):
    """The inputs of one world over ``T`` updates.  Without a script: tilt and loss of contact are two-state chains (runs shorter and
    longer than the tick limits), heights, positions and goals reach every bound, and in about one update in twelve one value of one
    input array — the arrays in turn — is NaN, +Inf, -Inf or a denormal."""
    out = {k: [] for k in INPUTS}
    tilted = airborne = False
    for k in range(T):
        s = None if script is None else script[k % len(script)]
        if s is None:
            tilted = rng.random() < (0.6 if tilted else 0.1)
            airborne = rng.random() < (0.7 if airborne else 0.1)
            u = rng.random()
            zk = "low" if u < 0.03 else "high" if u < 0.06 else "ok"
            far, near = rng.random() < 0.04, rng.random() < 0.05
            plant = rng.random() < 1 / 12
        else:
            tilted, airborne, zk, far, near, plant = s["tilt"], s["air"], s["z"], s["out"], s["goal"], s["bad"]
        theta = np.deg2rad(rng.uniform(65, 170) if tilted else rng.uniform(0, 50))
        axis, yaw = rng.uniform(0, 2 * np.pi), rng.uniform(-np.pi, np.pi)
        qt = np.array([np.cos(theta / 2), np.sin(theta / 2) * np.cos(axis), np.sin(theta / 2) * np.sin(axis), 0.0])
        qy = np.array([np.cos(yaw / 2), 0.0, 0.0, np.sin(yaw / 2)])
        quat = np.array([qy[0] * qt[0] - qy[3] * qt[3], qy[0] * qt[1] - qy[3] * qt[2], qy[0] * qt[2] + qy[3] * qt[1],
                         qy[0] * qt[3] + qy[3] * qt[0]])
        xy = rng.uniform(-9.5, 9.5, 2)
        if not near:                                                              # (keep off the goal unless it is meant)
            while np.hypot(*(xy - goal)) < 1.5:
                xy = rng.uniform(-9.5, 9.5, 2)
        if far:
            xy[rng.integers(0, 2)] = rng.choice([-1, 1]) * rng.uniform(10.5, 30)
        if near:
            xy = np.asarray(goal) + rng.uniform(-0.5, 0.5, 2)
        z = dict(ok=rng.uniform(0.6, 2.4), low=rng.uniform(-0.5, 0.45), high=rng.uniform(2.6, 5.0))[zk]
        sens = np.zeros((6, 4))
        sens[:, 0] = rng.random(6) < (0.3 if airborne else 0.7)
        sens[:, 1:] = rng.normal(0, 0.12 if airborne else 2.5, (6, 3))
        if airborne:
            sens[:, 1:] = np.clip(sens[:, 1:], -0.28, 0.28)                      # |F|^2 < 0.25: below every threshold
        elif script is not None:
            sens[2] = (1.0, 2.0, 2.0, 2.0)                                      # a scripted calm tick stands on a hind leg at least (|F|^2 = 12)
        vals = dict(pos=np.array([*xy, z]), quat=quat, vel=rng.normal(0, 3, 6), force=rng.normal(0, 6, n_act) * (rng.random(n_act) < 0.9),
                    qd=rng.normal(0, 6, n_act), sens=sens, ang=rng.normal(0, 1, n_q))
        vals = {name: np.asarray(v, dtype=f32) for name, v in vals.items()}
        if plant:
            name = INPUTS[k % len(INPUTS)] if script is None else INPUTS[(k // len(script)) % len(INPUTS)]
            flat = vals[name].reshape(-1)
            kinds = _KINDS if script is None else _KINDS[:3]
            flat[rng.integers(0, flat.size)] = kinds[rng.integers(0, len(kinds))]
        for name in INPUTS:
            out[name].append(vals[name])
    return {name: np.stack(v) for name, v in out.items()}


@functools.lru_cache(maxsize=None)
def input_run(n, T, n_act, n_q, seed=SEED):
    """The inputs of ``T`` updates of an ``n``-world batch: a dict of read-only float32 arrays ``pos (T, n, 3)``, ``quat (T, n, 4)``,
    ``vel (T, n, 6)``, ``force`` and ``qd`` ``(T, n, n_act)``, ``sens (T, n, 6, 4)``, ``ang (T, n, n_q)`` and the handle's own
    ``course`` and ``goal`` ``(n, 2)``.  World ``n - 1`` is the same world whatever ``n`` (its own random stream and the script);
    the others are drawn per index."""
    goals = np.random.default_rng([seed, 7]).uniform(-6, 6, (n, 2))
    goals[-1] = _LAST_GOAL
    angle = np.random.default_rng([seed, 8]).uniform(-np.pi, np.pi, n)
    angle[-1] = 0.7
    worlds = [_world(np.random.default_rng([seed, n_act, n_q, 0, i]), T, n_act, n_q, goals[i]) for i in range(n - 1)]
    worlds.append(_world(np.random.default_rng([seed, n_act, n_q, 1]), T, n_act, n_q, goals[-1], _script()))
    out = {name: np.stack([w[name] for w in worlds], axis=1) for name in INPUTS}
    out["course"] = np.stack([np.cos(angle), np.sin(angle)], axis=1).astype(f32)
    out["goal"] = goals.astype(f32)
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference_run(n, T, n_act, n_q, shared_course=False, params=PARITY, seed=SEED):
    """The specification's snapshots after each of ``T`` updates of :func:`input_run`'s inputs, with the coverage counts of
    :func:`coverage_add`; ``shared_course``: every world gets the course of world ``n - 1``."""
    run = input_run(n, T, n_act, n_q, seed)
    st = State(n, params, n_q, *standardisation(n_q))
    st.course[:] = run["course"][-1] if shared_course else run["course"]
    st.goal[:] = run["goal"]
    snaps, cover = [], coverage_start()
    for k in range(T):
        before = st.snapshot()
        st.update(*(run[name][k] for name in INPUTS))
        coverage_add(cover, before, st)
        snaps.append(st.snapshot())
    return snaps, cover


def coverage_start():
    return dict({name: 0 for name in REASONS}, truncated=0, grace_suppressed=0, tilt_limit=0, tilt_cut_short=0, airborne_limit=0,
                airborne_cut_short=0, fresh=0, progress=0)


def coverage_add(cover, before, st):
    """Counts, over the (update, world) pairs of one update (``before``: the snapshot it started from)."""
    p, last = st.p, st.last
    for name, bit in REASONS.items():
        cover[name] += int(((st.reason & bit) != 0).sum())
    cover["truncated"] += int(st.truncated.sum())
    cover["grace_suppressed"] += int((~last["bad"] & last["grace"] & ((last["raw"] & (TILTED | AIRBORNE | HEIGHT)) != 0)).sum())
    ok = ~last["bad"]
    cover["tilt_limit"] += int((ok & (last["tilt"] == p.tilt_ticks)).sum())
    cover["tilt_cut_short"] += int((ok & (before["tilt_count"] > 0) & (before["tilt_count"] < p.tilt_ticks) & (last["tilt"] == 0)).sum())
    cover["airborne_limit"] += int((ok & (last["air"] == p.airborne_ticks)).sum())
    cover["airborne_cut_short"] += int((ok & (before["airborne_count"] > 0) & (before["airborne_count"] < p.airborne_ticks)
                                        & (last["air"] == 0)).sum())
    cover["fresh"] += int(last["was_fresh"].sum())
    cover["progress"] += int((ok & (last["progress"] != 0)).sum())
