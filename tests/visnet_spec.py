"""The retinotopic visual network in numpy: the specification of ``flygym_amd/csrc/nmf_visnet.hip``
(``sensors.RetinotopicNetwork``), the networks of the parity cases and their inputs.  TEST INFRASTRUCTURE.

Build-defined and pinned by nothing: the reference snapshot holds no vision processing.  The statement of the model is
include/nmf.h (``nmf_visnet_update``).  Per world and eye, ``substeps`` times with the same readings, in float32::

    r[c][i] = v[c][i] > 0 ? v[c][i] : +0                                       (of the OLD state of every type)
    s = bias_c;  s = fmaf(in_w[c][0], x0_i, s);  s = fmaf(in_w[c][1], x1_i, s)
    for the edges into c in the caller's order, for the taps of each in the caller's order:
        j = neighbours[eye][t][i];  s = fmaf(w, j >= 0 ? r[pre][j] : +0, s)
    d = s - v[c][i];  m = a_c * d;  v[c][i] = v[c][i] + m                      (each rounded)

then ``S[c] = sum_i rint(min(r[c][i], 4) 2^16)`` as integers, ``pooled[c] = S[c] / (2^16 n_omm)`` (one float64 division of exact
operands rounded once to float32), and per world the signal ``t`` — the ``fmaf`` chain of ``steer_w_c (pooled[left][c] -
pooled[right][c])`` from +0 — and the optomotor rule of ``motion_spec.optomotor`` on ``gain t``.

:func:`update` is the specification proper; ``fmaf`` is the exact one of ``stabilizer_spec``.  :func:`update64` restates the rule
in float64 with exact coefficients and without the fixed-point step, and carries the bound :func:`update` is held to
(``tests/test_visnet_cpu.py``)."""
import functools
from dataclasses import dataclass

import numpy as np

from stabilizer_spec import fmaf

f32 = np.float32
U = 2.0 ** -24                               # unit roundoff of float32
CLAMP, SCALE = 4.0, 65536.0                  # a pooled term: clamped to 4, resolution 2^-16
MAX_TYPES, MAX_OMMATIDIA, MAX_CELLS, MAX_TABLE, MAX_EDGES, MAX_TAPS, MAX_SUBSTEPS = 32, 1024, 24576, 19, 512, 4096, 8
DEFAULTS = dict(gain=1.0, delta=0.8, base=1.0, drive_min=0.2, drive_max=1.2)
DT = 0.002
SEED = 20241021
N_TOTAL = 3                                  # the parity population: a batch of n worlds holds its LAST n worlds
WORLDS = (1, 3)
UPDATES = 4


@dataclass(frozen=True)
class Flat:
    """A flattened network: ``types`` (C, 5) float32 (bias, in_w0, in_w1, a, steer_w), ``edges`` (E, 2) int32 (post, pre), ``taps``
    (K, 2) int32 (edge, t), ``tap_w`` (K,) float32, ``tau`` (C,) float64 and the ``substeps`` its ``a`` was computed for."""
    types: np.ndarray
    edges: np.ndarray
    taps: np.ndarray
    tap_w: np.ndarray
    tau: np.ndarray
    substeps: int

    @property
    def n_types(self):
        return self.types.shape[0]

    def chains(self):
        """Per type the taps in the order the rule takes them: [(pre, t, w, tap index), ...]."""
        out = []
        for c in range(self.n_types):
            chain = []
            for e, (post, pre) in enumerate(self.edges.tolist()):
                if post == c:
                    chain += [(pre, int(self.taps[k, 1]), self.tap_w[k], k) for k in np.nonzero(self.taps[:, 0] == e)[0]]
            out.append(chain)
        return out


def coefficient(dt: float, tau, substeps: int) -> np.ndarray:
    """a = 1 - exp(-dt / (substeps tau)) in float64, rounded once to float32."""
    return (1.0 - np.exp(-np.float64(dt) / (substeps * np.asarray(tau, dtype=np.float64)))).astype(f32)


def flat(bias, in_w, steer_w, tau, edges, taps, tap_w, *, dt=DT, substeps=1) -> Flat:
    tau = np.asarray(tau, dtype=np.float64)
    types = np.stack([np.asarray(bias, dtype=f32), *np.asarray(in_w, dtype=f32).reshape(-1, 2).T, coefficient(dt, tau, substeps),
                      np.asarray(steer_w, dtype=f32)], axis=-1).astype(f32)
    out = Flat(types, np.asarray(edges, dtype=np.int32).reshape(-1, 2), np.asarray(taps, dtype=np.int32).reshape(-1, 2),
               np.asarray(tap_w, dtype=f32).reshape(-1), tau, int(substeps))
    for a in (out.types, out.edges, out.taps, out.tap_w, out.tau):
        a.setflags(write=False)
    return out


def both_eyes(neighbours) -> np.ndarray:
    """(T, n_omm) or (2, T, n_omm) -> (2, T, n_omm) int64."""
    nb = np.asarray(neighbours, dtype=np.int64)
    return np.stack([nb, nb]) if nb.ndim == 2 else nb


def new_state(n_worlds: int, n_types: int, n_omm: int, dtype=f32) -> dict:
    """Every eye fresh, the cells at zero (as a new handle)."""
    return dict(v=np.zeros((n_worlds, 2, n_types, n_omm), dtype=dtype), fresh=np.ones((n_worlds, 2), dtype=bool))


def reset(state: dict, mask=None) -> None:
    """Both eyes of the worlds of ``mask`` (default all) become fresh; nothing else changes."""
    if mask is None:
        state["fresh"][:] = True
    else:
        state["fresh"][np.asarray(mask) != 0] = True


def steer(pooled, steer_w, *, base, gain, delta, drive_min, drive_max, **_):
    """pooled (n, 2, C) float32 -> ``(signal (n,), drive (n, 2))`` float32.  ``base``: a scalar or an ``(n, 2)`` array."""
    pooled = np.asarray(pooled, dtype=f32)
    t = np.zeros(pooled.shape[0], dtype=f32)
    for c in range(pooled.shape[-1]):
        t = fmaf(f32(steer_w[c]), (pooled[:, 0, c] - pooled[:, 1, c]).astype(f32), t)
    t = np.where(t == 0, f32(0), t).astype(f32)                                        # (a zero is +0)
    g = (f32(gain) * t).astype(f32)
    with np.errstate(invalid="ignore"):
        q = (g.astype(np.float64) / (f32(1) + np.abs(g)).astype(f32).astype(np.float64)).astype(f32)
    d = f32(delta)
    o = np.stack([(f32(1) - (d * np.fmax(q, f32(0))).astype(f32)).astype(f32),
                  (f32(1) - (d * np.fmax(-q, f32(0))).astype(f32)).astype(f32)], axis=-1)
    b = np.broadcast_to(np.asarray(base, dtype=f32), o.shape)
    return t, np.fmin(np.fmax((b * o).astype(f32), f32(drive_min)), f32(drive_max)).astype(f32)


def update(state: dict, omm, net: Flat, neighbours, *, base=None, **params) -> dict:
    """One update of every world, in place on ``state``: ``dict(sums (n, 2, C) int32, pooled (n, 2, C), signal (n,), drive
    (n, 2))`` float32 and what the coverage assertions read — ``r_min``, ``r_max`` (C,) over every sub-step's new state,
    ``clamped`` (cells on the pooling clamp), ``missing`` (taps that met a missing neighbour), ``finite``.  ``omm`` (n, 2, n_omm, 2)
    float32; ``base`` None (the default), a scalar or an (n, 2) array."""
    p = {**DEFAULTS, **params}
    omm = np.asarray(omm, dtype=f32)
    n, _, n_omm, _ = omm.shape
    C = net.n_types
    nb = both_eyes(neighbours)
    assert C <= MAX_TYPES and n_omm <= MAX_OMMATIDIA and C * n_omm <= MAX_CELLS and nb.shape[1] <= MAX_TABLE
    assert len(net.edges) <= MAX_EDGES and len(net.taps) <= MAX_TAPS and 1 <= net.substeps <= MAX_SUBSTEPS
    bias, in_w0, in_w1, a, steer_w = net.types.T
    chains = net.chains()
    v = np.where(state["fresh"][:, :, None, None], bias[None, None, :, None], state["v"]).astype(f32)
    idx = np.where(nb < 0, n_omm, nb)                                                  # (the +0 cell behind every row)
    same = np.array_equal(idx[0], idx[1])                                              # (one gather serves both eyes)
    missing, finite = 0, True
    r_min, r_max = np.full(C, np.inf), np.full(C, -np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        for _ in range(net.substeps):
            r = np.concatenate([np.where(v > 0, v, f32(0)), np.zeros((n, 2, C, 1), dtype=f32)], axis=-1).astype(f32)
            new = np.empty_like(v)
            x0, x1 = omm[..., 0], omm[..., 1]                                          # (n, 2, n_omm)
            for c in range(C):
                s = np.full((n, 2, n_omm), bias[c], dtype=f32)
                s = fmaf(in_w0[c], x0, s)
                s = fmaf(in_w1[c], x1, s)
                for pre, t, w, _k in chains[c]:
                    s = fmaf(w, r[:, :, pre][:, :, idx[0, t]] if same else np.stack([r[:, e, pre][:, idx[e, t]] for e in range(2)], axis=1), s)
                    missing += int((nb[:, t] < 0).sum())
                finite &= bool(np.isfinite(s).all())
                d = (s - v[:, :, c]).astype(f32)
                m = (a[c] * d).astype(f32)
                new[:, :, c] = (v[:, :, c] + m).astype(f32)
            v = new
            rn = np.where(v > 0, v, f32(0))
            r_min, r_max = np.minimum(r_min, rn.min(axis=(0, 1, 3))), np.maximum(r_max, rn.max(axis=(0, 1, 3)))
        r = np.where(v > 0, v, f32(0)).astype(f32)
        capped = np.fmin(r, f32(CLAMP)).astype(f32)
        sums = np.rint((capped * f32(SCALE)).astype(f32)).astype(np.int64).sum(axis=-1)              # (n, 2, C)
    assert sums.max(initial=0) < 2 ** 29
    pooled = (sums.astype(np.float64) / np.float64(SCALE * n_omm)).astype(f32)
    signal, drive = steer(pooled, steer_w, **{**p, "base": p["base"] if base is None else base})
    state["v"], state["fresh"] = v, np.zeros_like(state["fresh"])
    finite &= bool(np.isfinite(v).all() and np.isfinite(drive).all())
    return dict(sums=sums.astype(np.int32), pooled=pooled, signal=signal, drive=drive, r_min=r_min, r_max=r_max,
                clamped=int((r >= f32(CLAMP)).sum()), missing=missing, finite=finite)


def update64(state: dict, omm, net: Flat, neighbours, *, dt=DT) -> dict:
    """The same rule in float64 with the exact coefficients ``-expm1(-dt / (substeps tau))`` and no fixed point, in place on
    ``state`` (of :func:`new_state` with ``dtype=np.float64``, plus ``bound``: 0 at the start): ``dict(pooled (n, 2, C) float64,
    bound)``.

    ``bound`` is what ``|v32 - v64|`` of :func:`update` cannot exceed, carried from sub-step to sub-step.  With E the bound on the
    old state, ReLU and the gathers being 1-Lipschitz, a type's new cell differs by at most

        (1 - a) E + a L E + a' (K + 2) u M + u (|d| + |m| + |v'|) + u |m|,      a' = a (1 + u)

    where L = sum |w| over the type's taps, K their number, M = |bias| + |in_w0 x0| + |in_w1 x1| + sum |w| (r_max + E) bounds every
    partial sum of the chain (each of its K + 2 fmaf rounds once: u M each), the three roundings of d, m and v' are u times their
    magnitudes, and the float32 coefficient is within u a of the exact one (u |m|).  Magnitudes are taken from this run, widened by
    E; the rounding terms are doubled for what is of second order in u, and the bound is the maximum over the types."""
    omm = np.asarray(omm, dtype=np.float64)
    n, _, n_omm, _ = omm.shape
    C = net.n_types
    nb = both_eyes(neighbours)
    bias, in_w0, in_w1, _, _ = net.types.astype(np.float64).T
    a = -np.expm1(-dt / (net.substeps * net.tau))
    chains = net.chains()
    v = np.where(state["fresh"][:, :, None, None], bias[None, None, :, None], state["v"])
    idx = np.where(nb < 0, n_omm, nb)
    E = float(state.get("bound", 0.0))
    for _ in range(net.substeps):
        r = np.concatenate([np.maximum(v, 0.0), np.zeros((n, 2, C, 1))], axis=-1)
        new = np.empty_like(v)
        worst = 0.0
        for c in range(C):
            s = bias[c] + in_w0[c] * omm[:, :, :, 0] + in_w1[c] * omm[:, :, :, 1]
            M = abs(bias[c]) + (np.abs(in_w0[c] * omm[..., 0]) + np.abs(in_w1[c] * omm[..., 1])).max()
            L = 0.0
            for pre, t, w, _k in chains[c]:
                s = s + np.float64(w) * np.stack([r[:, e, pre][:, idx[e, t]] for e in range(2)], axis=1)
                L += abs(float(w))
                M += abs(float(w)) * (r[:, :, pre].max() + E)
            d = s - v[:, :, c]
            m = a[c] * d
            new[:, :, c] = v[:, :, c] + m
            mag = np.abs(d).max() + 2.0 * np.abs(m).max() + np.abs(new[:, :, c]).max() + 4.0 * E * (1.0 + L)
            worst = max(worst, (1.0 - a[c]) * E + a[c] * L * E + 2.0 * (a[c] * (1.0 + U) * (len(chains[c]) + 2) * U * M + U * mag))
        v, E = new, worst
    state["v"], state["fresh"], state["bound"] = v, np.zeros_like(state["fresh"]), E
    pooled = np.minimum(np.maximum(v, 0.0), CLAMP).mean(axis=-1)
    return dict(pooled=pooled, bound=E)


# ---- the parity cases ----

def hex_id_map(radius: int, side: int = 64) -> np.ndarray:
    from flygym_amd.sensors import make_ommatidia_id_map

    return make_ommatidia_id_map(side, side, radius)


@functools.lru_cache(maxsize=None)
def retina(name: str):
    """'default' (721 ommatidia), 'seven' (a centre and its six neighbours), 'one' (one ommatidium), 'square' (32 x 32 = 1024, one
    pixel each: no hexagonal lattice)."""
    from flygym_amd.sensors import Retina

    if name == "default":
        return Retina()
    if name == "seven":
        return Retina(id_map=hex_id_map(1))
    if name == "one":
        return Retina(id_map=np.ones((3, 3), dtype=np.int16))
    assert name == "square"
    return Retina(id_map=np.arange(1, 1025, dtype=np.int16).reshape(32, 32))


def _types(rng, C):
    """bias and in_w of opposite signs, |in_w| > |bias|: over readings in [0, 1) every type is driven above and below zero."""
    sign = np.where(rng.random(C) < 0.5, -1.0, 1.0)
    bias = sign * rng.uniform(0.1, 0.3, C)
    in_w = -sign[:, None] * rng.uniform(0.5, 1.0, (C, 2))
    return bias, in_w, rng.uniform(-1.0, 1.0, C), rng.uniform(0.004, 0.05, C)


@functools.lru_cache(maxsize=None)
def case(name: str, substeps: int = 1):
    """``(Flat, neighbours, retina name)`` of a parity case.

    smallest  one type, no edges, the 1-cell retina, T = 1
    ring      two types, a self edge and mutual edges, the 7-cell retina, T = 7
    ragged    five types on the default retina, T = 19: type 1 has no incoming edge, type 3 three incoming edges of 1, 7 and 19
              taps, taps repeated and out of order
    widest    32 types on the default retina: 512 edges and 4096 taps, the limits
    square    24 types x 1024 ommatidia with a random table of 19 rows that contains -1: the largest LDS image
    """
    rng = np.random.default_rng([SEED, sum(map(ord, name))])
    if name == "smallest":
        bias, in_w, steer_w, tau = _types(rng, 1)
        return flat(bias, in_w, steer_w, tau, [], [], [], substeps=substeps), retina("one").hex_neighbours(0)[0], "one"
    if name == "ring":
        bias, in_w, steer_w, tau = _types(rng, 2)
        edges = [(0, 0), (1, 0), (0, 1)]
        taps = [(0, 0), (0, 3), (1, 1), (1, 2), (1, 4), (2, 6), (2, 5), (2, 0)]
        return (flat(bias, in_w, steer_w, tau, edges, taps, rng.uniform(-0.3, 0.3, len(taps)), substeps=substeps),
                retina("seven").hex_neighbours(1)[0], "seven")
    if name == "ragged":
        bias, in_w, steer_w, tau = _types(rng, 5)
        edges = [(3, 0), (0, 4), (3, 3), (2, 1), (4, 2), (3, 1), (0, 0)]
        taps = [(0, 5)]                                                        # edge 0 into type 3: one tap
        taps += [(2, t) for t in (6, 0, 3, 3, 1, 5, 2)]                        # edge 2: seven, one row twice, out of order
        taps += [(1, 18), (3, 7), (3, 7), (4, 12), (6, 9), (6, 0)]
        taps += [(5, t) for t in rng.permutation(19).tolist()]                 # edge 5: all nineteen, shuffled
        taps += [(1, 2), (4, 0)]                                               # (taps of earlier edges after later ones)
        return (flat(bias, in_w, steer_w, tau, edges, taps, rng.uniform(-0.15, 0.15, len(taps)), substeps=substeps),
                retina("default").hex_neighbours(2)[0], "default")
    C = 32 if name == "widest" else 24
    assert name in ("widest", "square")
    bias, in_w, steer_w, tau = _types(rng, C)
    edges = np.stack([rng.integers(0, C, MAX_EDGES), rng.integers(0, C, MAX_EDGES)], axis=-1)
    taps = np.stack([rng.integers(0, MAX_EDGES, MAX_TAPS), rng.integers(0, MAX_TABLE, MAX_TAPS)], axis=-1)
    net = flat(bias, in_w, steer_w, tau, edges, taps, rng.uniform(-1.0, 1.0, MAX_TAPS) * (1.5 * C / MAX_TAPS), substeps=substeps)
    if name == "widest":
        return net, retina("default").hex_neighbours(2)[0], "default"
    table = rng.integers(-1, 1024, (2, MAX_TABLE, 1024)).astype(np.int32)     # (a table per eye)
    table[:, 0] = np.arange(1024)
    return net, table, "square"


@functools.lru_cache(maxsize=None)
def readings(n_omm: int, seed: int = 0):
    """(UPDATES, N_TOTAL, 2, n_omm, 2) float32, read-only; a reading sits in one channel, the other is 0.  World 0 reads up to 60
    (cells far beyond the pooling clamp), the others uniform in [0, 1); the left eye of world 1 repeats its first frame."""
    rng = np.random.default_rng([SEED, n_omm, seed])
    r = rng.random((UPDATES, N_TOTAL, 2, n_omm)).astype(f32)
    r[:, 0] *= f32(60.0)
    r[:, 1, 0] = r[0, 1, 0]
    pale = rng.random((N_TOTAL, 2, n_omm)) < 0.3
    omm = np.stack([np.where(pale, 0, r), np.where(pale, r, 0)], axis=-1).astype(f32)
    omm.setflags(write=False)
    return omm


@functools.lru_cache(maxsize=None)
def bases():
    """(N_TOTAL, 2) float32: world 0 below drive_min and above drive_max, the others inside."""
    b = np.array([[0.1, 1.5], [0.9, 1.0], [1.1, 0.7]], dtype=f32)
    b.setflags(write=False)
    return b


PARAMS = dict(gain=30.0, delta=0.7, base=0.95)


def run(net: Flat, neighbours, n_omm: int, n: int, *, reset_at=None, reset_mask=None):
    """The parity protocol on the last ``n`` worlds of the population: UPDATES updates — the scalar base, then the base tensor, ...
    alternating — with a masked reset before update ``reset_at``.  Returns the list of ``(state copy, outputs)`` per update."""
    omm, base = readings(n_omm)[:, N_TOTAL - n:], bases()[N_TOTAL - n:]
    state = new_state(n, net.n_types, n_omm)
    out = []
    for k in range(UPDATES):
        if reset_at == k:
            reset(state, reset_mask)
        got = update(state, omm[k], net, neighbours, **{**PARAMS, "base": base if k % 2 else PARAMS["base"]})
        out.append((dict(v=state["v"].copy(), fresh=state["fresh"].copy()), got))
    return out
