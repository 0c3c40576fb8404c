"""The plume navigator's specification in numpy (the kernel is ``flygym_amd/csrc/nmf_navigator.hip``, the class
``flygym_amd.controllers.PlumeNavigator``, the statement of the model ``include/nmf.h``, ``nmf_navigator_update``).

Written from the definition, one update at a time, every world at once.  Everything is float32 and every operation is rounded on its
own; every right-hand side is the old state except that the probabilities use the filters just updated::

    s = I[2] + I[3];  now = s > threshold;  e = now and not above;  above <- now;  encounters += e
    k_stop <- k_stop * decay_stop + e;  k_walk <- k_walk * decay_walk + e;  freq <- freq * decay_freq + (e ? inv_tau_freq : 0)
    ax = 1 - 2 * (qy * qy + qz * qz);  ay = 2 * (qx * qy + qw * qz);  cross = ay * wx - ax * wy
    u_m = plume_spec.uniforms(seed, first_world + w, ticks, 8 + m) * 2^-24,  m = 0, 1, 2
    p_stop = c01(dt * (lambda_ws0 + dlambda_ws * k_stop));  p_walk = c01(dt * (lambda_sw0 + dlambda_sw * k_walk))
    p_turn = c01(dt * lambda_turn);  p_up = clamp(p_up0 + up_gain * freq, p_up_min, p_up_max)
    a turn: remaining -= 1; at <= 0 -> WALK
    WALK: u_0 < p_stop -> STOP;  else u_1 < p_turn -> remaining = turn_ticks, towards = u_2 < p_up ? upwind : downwind,
          TURN_LEFT when (towards upwind) == (cross > 0), else TURN_RIGHT
    STOP: u_0 < p_walk -> WALK
    ticks += 1;  drive = the row of the new state

The clamps are comparisons (``np.where``), so a NaN would pass through as in the kernel.  ``decay_*`` and ``inv_tau_freq`` are
float32 numbers the caller computed (``flygym_amd.controllers.navigator_constants``): no ``exp`` is taken here.

The second half of the module is the input generator and the settings the GPU parity tests use; ``tests/test_navigator_cpu.py``
asserts on the specification alone that they exercise every transition.
"""
import functools
from dataclasses import dataclass

import numpy as np

import plume_spec

WALK, STOP, TURN_LEFT, TURN_RIGHT = 0, 1, 2, 3
FIELDS = ("state", "remaining", "above", "k_stop", "k_walk", "freq", "ticks", "encounters", "drive")
f32 = np.float32


@dataclass(frozen=True)
class Params:
    """``nmf_navigator_params`` without the indices: float32 values, ``turn_ticks`` an int."""

    dt: float
    threshold: float
    decay_stop: float
    decay_walk: float
    decay_freq: float
    inv_tau_freq: float
    turn_ticks: int
    lambda_ws0: float = 0.78
    dlambda_ws: float = -0.61
    lambda_sw0: float = 0.29
    dlambda_sw: float = 0.41
    lambda_turn: float = 1.33
    p_up0: float = 0.5
    up_gain: float = 0.15
    p_up_min: float = 0.05
    p_up_max: float = 0.95
    walk_drive: tuple = (1.0, 1.0)
    stop_drive: tuple = (0.0, 0.0)
    turn_drive: tuple = (-0.4, 1.2)

    def __post_init__(self):
        for name, value in list(self.__dict__.items()):
            if name == "turn_ticks":
                value = int(value)
            elif isinstance(value, tuple):
                value = (f32(value[0]), f32(value[1]))
            else:
                value = f32(value)
            object.__setattr__(self, name, value)

    @classmethod
    def from_struct(cls, p):
        """From the ctypes mirror ``flygym_amd.controllers._NavigatorParams`` of a live navigator."""
        pairs = {k: (p.__getattribute__(k)[0], p.__getattribute__(k)[1]) for k in ("walk_drive", "stop_drive", "turn_drive")}
        return cls(**{k: getattr(p, k) for k in cls.__dataclass_fields__ if k not in pairs}, **pairs)


def clamp(x, lo, hi):
    """``x < lo ? lo : (x > hi ? hi : x)`` on float32 arrays."""
    return np.where(x < lo, f32(lo), np.where(x > hi, f32(hi), x)).astype(f32)


def draws(seed, world, tick):
    """The three uniform draws ``(3, n)`` float32 of the worlds ``world`` (global indices) at the tick counters ``tick``."""
    return np.stack([plume_spec.uniforms(seed, world, tick, 8 + m).astype(f32) * f32(2.0 ** -24) for m in range(3)])


class State:
    """The state of ``n`` worlds.  After an update ``last`` holds what it decided, per world: ``e``, ``p_stop``, ``p_walk``,
    ``p_turn``, ``p_up``, ``cross_positive``, ``decided`` (a turn began) and ``upwind`` (it went towards upwind)."""

    def __init__(self, n, params, seed=0, first_world=0):
        self.n, self.p, self.seed, self.first_world = int(n), params, int(seed) & 0xFFFFFFFF, int(first_world)
        self.state = np.zeros(n, dtype=np.int32)
        self.remaining = np.zeros(n, dtype=np.int32)
        self.above = np.zeros(n, dtype=np.uint8)
        self.k_stop, self.k_walk, self.freq = (np.zeros(n, dtype=f32) for _ in range(3))
        self.ticks = np.zeros(n, dtype=np.uint32)
        self.encounters = np.zeros(n, dtype=np.int32)
        self.drive = np.zeros((n, 2), dtype=f32)
        self.last = {}
        self.reset()

    def reset(self, mask=None):
        m = np.ones(self.n, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
        for name in FIELDS[:-1]:
            getattr(self, name)[m] = 0
        self.drive[m] = self.p.walk_drive

    def update(self, odor, wind, quat, odor_dim=0):
        """``odor`` ``(n, n_dims, 4)``, ``wind`` ``(n, 2)`` or one shared row ``(1, 2)`` / ``(2,)``, ``quat`` ``(n, 4)`` (w, x, y, z)."""
        p, n = self.p, self.n
        I = np.asarray(odor, dtype=f32).reshape(n, -1, 4)[:, odor_dim]
        wind = np.broadcast_to(np.asarray(wind, dtype=f32).reshape(-1, 2), (n, 2))
        qw, qx, qy, qz = np.asarray(quat, dtype=f32).reshape(n, 4).T
        with np.errstate(invalid="ignore", over="ignore"):
            s = I[:, 2] + I[:, 3]
            now = s > p.threshold
            e = now & (self.above == 0)
            ef = e.astype(f32)
            k_stop = self.k_stop * p.decay_stop + ef
            k_walk = self.k_walk * p.decay_walk + ef
            freq = self.freq * p.decay_freq + np.where(e, p.inv_tau_freq, f32(0))
            ax = f32(1) - f32(2) * (qy * qy + qz * qz)
            ay = f32(2) * (qx * qy + qw * qz)
            cross = ay * wind[:, 0] - ax * wind[:, 1]
            up_left = cross > 0
        u = draws(self.seed, self.first_world + np.arange(n), self.ticks)
        p_stop = clamp(p.dt * (p.lambda_ws0 + p.dlambda_ws * k_stop), 0, 1)
        p_walk = clamp(p.dt * (p.lambda_sw0 + p.dlambda_sw * k_walk), 0, 1)
        p_turn = clamp(np.full(n, p.dt * p.lambda_turn, dtype=f32), 0, 1)
        p_up = clamp(p.p_up0 + p.up_gain * freq, p.p_up_min, p.p_up_max)
        assert all(a.dtype == f32 for a in (s, k_stop, k_walk, freq, cross, u, p_stop, p_walk, p_turn, p_up))

        walking, stopped = self.state == WALK, self.state == STOP
        turning = ~walking & ~stopped
        stop = walking & (u[0] < p_stop)
        decided = walking & ~stop & (u[1] < p_turn)
        upwind = u[2] < p_up
        nxt = self.state.copy()
        nxt[stop] = STOP
        nxt[decided] = np.where(upwind == up_left, TURN_LEFT, TURN_RIGHT)[decided]
        nxt[stopped & (u[0] < p_walk)] = WALK
        remaining = self.remaining.copy()
        remaining[decided] = p.turn_ticks
        remaining[turning] -= 1
        nxt[turning & (remaining <= 0)] = WALK

        self.state, self.remaining, self.above = nxt.astype(np.int32), remaining.astype(np.int32), now.astype(np.uint8)
        self.k_stop, self.k_walk, self.freq = k_stop, k_walk, freq
        self.ticks = self.ticks + np.uint32(1)
        self.encounters = (self.encounters + e).astype(np.int32)
        rows = np.array([p.walk_drive, p.stop_drive, p.turn_drive, p.turn_drive[::-1]], dtype=f32)
        self.drive = rows[np.where((nxt < 0) | (nxt > 3), TURN_LEFT, nxt)]
        self.last = dict(e=e, p_stop=p_stop, p_walk=p_walk, p_turn=p_turn, p_up=p_up, cross_positive=up_left, decided=decided,
                         upwind=upwind & decided)

    def snapshot(self):
        return {name: np.copy(getattr(self, name)) for name in FIELDS}


# ---- what the GPU parity tests run: settings, inputs, reference runs -------------------------------------------------------

# (n_worlds, updates): one world, one lane past a wave, one lane past a workgroup; world n - 1 of each has the global index LAST
CASES = ((1, 300), (65, 120), (257, 60))
LAST = 256
SEED = 21
PARITY = Params(dt=0.05, threshold=0.1, decay_stop=np.exp(-0.05 / 0.2), decay_walk=np.exp(-0.05 / 0.52), decay_freq=np.exp(-0.05 / 2.0),
                inv_tau_freq=0.5, turn_ticks=3, lambda_ws0=4 * 0.78, dlambda_ws=4 * -0.61, lambda_sw0=4 * 0.29, dlambda_sw=4 * 0.41,
                lambda_turn=4 * 1.33, p_up0=0.5, up_gain=0.15, p_up_min=0.05, p_up_max=0.95, turn_drive=(0.4, 1.2))
PARITY_TIMES = dict(tick_s=0.05, tau_stop=0.2, tau_walk=0.52, tau_freq=2.0, turn_duration=0.15)      # PARITY's, as the class takes them


def first_world(n):
    return LAST + 1 - n


def inputs(seed, k, n, n_dims=2):
    """Inputs of update ``k`` for an ``n``-world batch: ``(odor (n, n_dims, 4), wind (n, 2), quat (n, 4))`` float32.  World ``n - 1``
    is the same world whatever ``n`` (its own random stream), the others are drawn per index.  Each reading is a value in 0..0.3
    with probability 1/4, else 0 (against a threshold of 0.1); the wind is normal with sigma 30; the attitude is random, tilted up
    to some 30 degrees, any yaw.  About one entry in 60 of the antennae and of the wind is NaN, +Inf or -Inf."""
    def draw(rng, m):
        odor = np.where(rng.random((m, n_dims, 4)) < 0.25, rng.uniform(0.0, 0.3, (m, n_dims, 4)), 0.0).astype(np.float32)
        wind = rng.normal(0.0, 30.0, (m, 2)).astype(np.float32)
        q = rng.normal(size=(m, 4)) * np.array([1.0, 0.25, 0.25, 1.0])
        quat = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
        odd = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)
        bad = rng.random(odor.shape) < 1 / 60
        odor[bad] = odd[rng.integers(0, 3, int(bad.sum()))]
        bad = rng.random(wind.shape) < 1 / 60
        wind[bad] = odd[rng.integers(0, 3, int(bad.sum()))]
        return odor, wind, quat

    a = draw(np.random.default_rng([seed, k, 0]), n - 1)
    b = draw(np.random.default_rng([seed, k, 1]), 1)
    return tuple(np.concatenate([u, v]) for u, v in zip(a, b))


@functools.lru_cache(maxsize=None)
def input_run(n, T, seed=SEED, n_dims=2):
    """The inputs of ``T`` updates stacked: ``(odor (T, n, n_dims, 4), wind (T, n, 2), quat (T, n, 4))``, read-only."""
    out = tuple(np.stack(a) for a in zip(*(inputs(seed, k, n, n_dims) for k in range(T))))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference_run(n, T, shared_wind=False, seed=SEED, odor_dim=1, params=PARITY):
    """The specification's snapshots after each of ``T`` updates of an ``n``-world batch whose world ``n - 1`` has the global index
    LAST, with the coverage counts of :func:`coverage`; ``shared_wind``: every world gets the wind row of world ``n - 1``."""
    odor, wind, quat = input_run(n, T, seed)
    st = State(n, params, seed=seed, first_world=first_world(n))
    snaps, cover = [], coverage_start()
    for k in range(T):
        before = st.state.copy()
        st.update(odor[k], wind[k, -1] if shared_wind else wind[k], quat[k], odor_dim)
        coverage_add(cover, before, st)
        snaps.append(st.snapshot())
    return snaps, cover


def coverage_start():
    return dict(walk_stop=0, stop_walk=0, walk_left=0, walk_right=0, left_walk=0, right_walk=0, upwind=0, downwind=0, p_up_inside=0,
                encounters=0)


def coverage_add(cover, before, st):
    """Counts the transitions of one update (``before``: the states it started from)."""
    after, last, p = st.state, st.last, st.p
    for name, a, b in (("walk_stop", WALK, STOP), ("stop_walk", STOP, WALK), ("walk_left", WALK, TURN_LEFT), ("walk_right", WALK, TURN_RIGHT),
                       ("left_walk", TURN_LEFT, WALK), ("right_walk", TURN_RIGHT, WALK)):
        cover[name] += int(((before == a) & (after == b)).sum())
    cover["upwind"] += int(last["upwind"].sum())
    cover["downwind"] += int((last["decided"] & ~last["upwind"]).sum())
    cover["p_up_inside"] += int((last["decided"] & (last["p_up"] > p.p_up_min) & (last["p_up"] < p.p_up_max)).sum())
    cover["encounters"] += int(last["e"].sum())
