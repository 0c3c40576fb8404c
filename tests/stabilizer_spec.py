"""Numpy specification of the head stabilizer (``flygym_amd/csrc/nmf_stabilizer.hip``, ``flygym_amd.controllers.HeadStabilizer``;
the model is stated in include/nmf.h, ``nmf_stabilizer_update``), the networks of the parity cases and their inputs.

Per world, in float32::

    x[k]      = (q[dof[k]] - mean[k]) * inv_std[k]                                  (subtract, round, multiply, round)
    m_l       = fmaf(Fz, Fz, fmaf(Fy, Fy, Fx * Fx));  x[n_q + l] = found_l > 0 and m_l > thr2[l]
    a[j] = b[j];  for k ascending: a[j] = fmaf(W[j, k], h[k], a[j]);  h = a > 0 ? a : 0;  the last layer: y = a
    y[j]      = y[j] < lo[j] ? lo[j] : (y[j] > hi[j] ? hi[j] : y[j])

``fmaf`` here is an exact float32 fused multiply-add without ``math.fma``: the product of two float32 numbers is exact in float64
(48 bits), the float64 sum with the addend is taken with an error-free TwoSum, a sum that is not exact is rounded to odd (of the
two float64 neighbours of the true value the one with an odd last bit), and the cast to float32 then rounds once: float64 carries
29 bits more than float32, and rounding to odd followed by rounding to nearest equals rounding the true value to nearest whenever
the wider format has at least two bits more.  ``tests/test_stabilizer_cpu.py`` compares it with libm's ``fmaf`` bit for bit.
"""
import functools
from dataclasses import dataclass

import numpy as np

F32 = np.float32
SEED = 20240611
N_TOTAL = 257                      # the parity population: a batch of n worlds holds its LAST n worlds
WORLDS = (1, 65, 257)              # one world, one lane past a wave, one past four waves
UPDATES = 4
N_DOF = 66                         # joint dofs of make_model()'s LEGS_ONLY fly (qpos columns 7 .. 72); 42 of them are actuated
THR = (0.5, 1.0, 3.0)              # contact force thresholds of the front, middle and hind legs
LEG_PAIR = (0, 1, 2, 0, 1, 2)      # lf lm lh rf rm rh


def fmaf(a, b, c):
    """Exact float32 fused multiply-add of float32 arrays: round(a * b + c) with one rounding."""
    a, b, c = (np.asarray(v, dtype=F32) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)                  # exact
        c64 = c.astype(np.float64)
        s = p + c64
        bb = s - p
        err = (p - (s - bb)) + (c64 - bb)                                # TwoSum: p + c64 = s + err exactly
        inexact = np.isfinite(s) & (err != 0)
        even = (s.view(np.int64) & 1) == 0
        other = np.where(err > 0, np.nextafter(s, np.inf), np.nextafter(s, -np.inf))
        s = np.where(inexact & even, other, s)                            # round to odd
        return s.astype(F32)


@dataclass(frozen=True)
class Net:
    name: str
    dof: np.ndarray            # (n_q,) int32 indices into the joint dofs
    mean: np.ndarray           # (n_q,) float32
    std: np.ndarray            # (n_q,) float32
    contacts: bool
    layers: tuple              # ((W (n_out_i, n_in_i) float32, b (n_out_i,) float32), ...)

    @property
    def inv_std(self):
        return (1.0 / self.std.astype(np.float64)).astype(F32)

    @property
    def thr2(self):
        return np.array([float(THR[p]) ** 2 for p in LEG_PAIR], dtype=F32)

    @property
    def n_q(self):
        return len(self.dof)

    @property
    def n_in(self):
        return self.n_q + (6 if self.contacts else 0)

    @property
    def n_out(self):
        return self.layers[-1][0].shape[0]


# name: (n_q, contacts, hidden widths, outputs).  "default" is 48 -> 32 -> 32 -> 2 on the fly's 42 actuated leg dofs (the class's
# default inputs); "smallest" one joint angle, one hidden unit, one output; "ragged" sits at the limits with widths that cross any
# blocking by 2, 4, 8 or 32 (all 66 joint dofs, shuffled); "widest" has the most inputs the kernel takes, 250 + 6 (dofs repeat).
ARCHITECTURES = {"default": (42, True, (32, 32), 2), "smallest": (1, False, (1,), 1), "ragged": (66, True, (33, 64, 7), 8),
                 "widest": (250, True, (8,), 1)}
PARITY = ("default", "smallest", "ragged")


def actuated_dofs():
    """Indices, among the joint dofs of ``make_model()``'s fly, of those with a position actuator, in the actuators' order."""
    from flygym_amd import make_model

    fly, _, _ = make_model()
    names = [d.name for d in fly.get_jointdofs_order()]
    assert len(names) == N_DOF
    return np.array([names.index(d.name) for d in fly.get_actuated_jointdofs_order("position")])


@functools.lru_cache(maxsize=None)
def network(name) -> Net:
    n_q, contacts, hidden, n_out = ARCHITECTURES[name]
    rng = np.random.default_rng([SEED, sorted(ARCHITECTURES).index(name)])
    dof = {"default": actuated_dofs, "ragged": lambda: rng.permutation(N_DOF)}.get(name, lambda: rng.integers(0, N_DOF, n_q))().astype(np.int32)
    assert dof.shape == (n_q,)
    mean = rng.normal(0.0, 0.5, n_q).astype(F32)
    std = rng.uniform(0.5, 1.5, n_q).astype(F32)
    sizes = [n_q + (6 if contacts else 0), *hidden, n_out]
    # Random weights; each unit's bias puts a random 30 % .. 70 % quantile of its pre-activation over the population (estimated
    # with a plain float64 pass) at zero, so that every hidden unit is both active and clipped somewhere — which the CPU tests then
    # check on the specification itself.
    q, sd = _population(UPDATES)
    h = (q.reshape(-1, N_DOF)[:, dof].astype(np.float64) - mean) / std
    if contacts:
        s = sd.reshape(-1, 6, 16).astype(np.float64)
        h = np.concatenate([h, (s[:, :, 0] > 0) & ((s[:, :, 1:4] ** 2).sum(axis=2) > np.array(THR)[list(LEG_PAIR)] ** 2)], axis=1)
    layers = []
    for a, b in zip(sizes[:-1], sizes[1:]):
        W = rng.normal(0.0, np.sqrt(2.0 / a), (b, a)).astype(F32)
        pre = h @ W.astype(np.float64).T
        bias = np.array([-np.quantile(col, rng.uniform(0.3, 0.7)) for col in pre.T]).astype(F32)
        layers.append((W, bias))
        h = np.maximum(pre + bias, 0.0)
    return Net(name, dof, mean, std, contacts, tuple(layers))


@functools.lru_cache(maxsize=None)
def _population(T):
    """Joint angles (T, N_TOTAL, N_DOF) and sensordata (T, N_TOTAL, 96) of the whole parity population."""
    rng = np.random.default_rng([SEED, 1000 + T])
    q = rng.normal(0.0, 1.0, (T, N_TOTAL, N_DOF)).astype(F32)
    sd = rng.normal(0.0, 1.0, (T, N_TOTAL, 6, 16)).astype(F32)
    sd[..., 0] = rng.integers(0, 3, (T, N_TOTAL, 6)).astype(F32)                    # contacts found: 0, 1 or 2
    direction = rng.normal(0.0, 1.0, (T, N_TOTAL, 6, 3))
    direction /= np.linalg.norm(direction, axis=-1, keepdims=True)
    size = np.array(THR)[list(LEG_PAIR)] * rng.uniform(0.2, 2.0, (T, N_TOTAL, 6))  # around the leg's threshold
    sd[..., 1:4] = (direction * size[..., None]).astype(F32)
    q.setflags(write=False); sd.setflags(write=False)
    return q, sd.reshape(T, N_TOTAL, 96)


def input_run(n, T=UPDATES):
    """The inputs of the last ``n`` worlds of the population: joint angles (T, n, N_DOF), sensordata (T, n, 96), float32."""
    q, sd = _population(T)
    return q[:, N_TOTAL - n:], sd[:, N_TOTAL - n:]


def forward(net: Net, q, sd, lo=None, hi=None):
    """The specification.  ``q`` (..., N_DOF) joint angles, ``sd`` (..., 96); returns ``(y, trace)``: the outputs (..., n_out)
    (clamped when ``lo`` / ``hi`` are given) and a dict with the inputs ``x``, the flags, each hidden layer's pre-activations, the
    unclamped outputs and the smallest nonzero / largest magnitude among all intermediates."""
    q, sd = np.asarray(q, dtype=F32), np.asarray(sd, dtype=F32)
    extremes = [np.inf, 0.0]

    def note(a):
        mags = np.abs(a)
        if (mags > 0).any():
            extremes[0] = min(extremes[0], float(mags[mags > 0].min()))
        extremes[1] = max(extremes[1], float(mags.max()))
        return a

    x = note(note(q[..., net.dof] - net.mean) * net.inv_std)
    trace = {}
    if net.contacts:
        s = sd.reshape(*sd.shape[:-1], 6, 16)
        fx, fy, fz = s[..., 1], s[..., 2], s[..., 3]
        m = note(fmaf(fz, fz, note(fmaf(fy, fy, note(fx * fx)))))
        flags = (s[..., 0] > 0) & (m > net.thr2)
        trace["found_below"] = (s[..., 0] > 0) & ~(m > net.thr2)
        trace["flags"] = flags
        x = np.concatenate([x, flags.astype(F32)], axis=-1)
    trace["x"] = x
    h = x
    trace["hidden"] = []
    for i, (W, b) in enumerate(net.layers):
        a = np.broadcast_to(b, (*h.shape[:-1], len(b))).astype(F32)
        for k in range(W.shape[1]):
            a = note(fmaf(W[:, k], h[..., k:k + 1], a))
        if i + 1 < len(net.layers):
            trace["hidden"].append(a)
            h = np.where(a > 0, a, F32(0.0)).astype(F32)
    trace["unclamped"] = a
    y = a
    if lo is not None:
        lo, hi = np.asarray(lo, dtype=F32), np.asarray(hi, dtype=F32)
        y = np.where(y < lo, lo, np.where(y > hi, hi, y)).astype(F32)
    trace["smallest_nonzero"], trace["largest"] = extremes
    return y, trace


@functools.lru_cache(maxsize=None)
def bounds(name):
    """``(lo, hi)`` float32 per output: the 30 % and 70 % quantiles of the distinct values of the specification's unclamped
    outputs over the whole population (distinct: with one hidden unit every world in which it is clipped gives the output bias),
    so that every output is clamped at both ends and left alone in between — a choice of inputs, made on the specification alone."""
    _, trace = forward(network(name), *input_run(N_TOTAL))
    u = trace["unclamped"].reshape(-1, network(name).n_out).astype(np.float64)
    lo, hi = (np.array([np.quantile(np.unique(col), q) for col in u.T]).astype(F32) for q in (0.3, 0.7))
    return lo, hi


@functools.lru_cache(maxsize=None)
def reference_run(name, n, T=UPDATES):
    """``(y (T, n, n_out), trace)`` of the last ``n`` worlds; read-only."""
    y, trace = forward(network(name), *input_run(n, T), *bounds(name))
    y.setflags(write=False)
    return y, trace


def relu_mlp(layers, x):
    """A plain float64 forward pass (for the tests of ``fit``)."""
    h = np.asarray(x, dtype=np.float64)
    for i, (W, b) in enumerate(layers):
        h = h @ np.asarray(W, dtype=np.float64).T + np.asarray(b, dtype=np.float64)
        if i + 1 < len(layers):
            h = np.maximum(h, 0.0)
    return h
