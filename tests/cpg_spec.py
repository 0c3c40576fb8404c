"""The closed-loop tripod CPG's specification in numpy (the kernel is ``flygym_amd/csrc/nmf_cpg.hip``, the class
``flygym_amd.controllers.TurningCPG``).

Written from the definition, one step at a time, vectorised over the worlds only.  Six coupled phase oscillators per world, legs
in ``LEGS`` order; state: phase ``theta`` in cycles in [0, 1) and magnitude ``r``; input: the drive ``d = (d_left, d_right)``.
The row of a step is computed from the state before its update, and every right-hand side uses the old state::

    R_l = |d_side(l)|       nu_l = nu * sign(d_side(l))                       (sign(0) = 0: that side holds its phase)
    x = theta_l * n_bins;  i0 = floor(x) mod n_bins;  f = x - floor(x)
    c = (1 - f) * cycle[i0, col] + f * cycle[(i0 + 1) mod n_bins, col]
    target[col] = c + (r_l - 1) * (c - mean[col])                             (mean: the cycle's mean over its bins)
    adhesion[l] = on if stance[i0, l] else off                                (six optional columns)
    theta_l <- (theta_l + dt * (nu_l + (1 / 2 pi) * sum_{j != l} r_j * w * sin(2 pi (theta_j - theta_l) - phi_lj))) mod 1
    r_l     <- r_l + dt * a * (R_l - r_l)                                     (phi_lj = b_j - b_l, b = TRIPOD_PHASE_BIAS)

``dtype=np.float64``: everything in float64.  ``dtype=np.float32`` is the float32 flavour: the phase, its bin position ``x`` and
its increment ``dt * (nu_l + S / 2 pi)`` stay float64 (a float32 phase wrapped every step drifts 4e-5 cycles in 2500 steps, and
``dt * nu`` rounded to float32 still 2e-7); the coupling sum ``S`` with its sines, the magnitudes, ``f`` and the rows are float32.
The kernel is this flavour with one refinement: it sums the magnitudes' Euler steps in float64 and rounds them to float32 where
they are read (float32 sums wander up to 17 ulp from the float64 recurrence in 400 steps).
"""
import numpy as np

from flygym_amd.anatomy import LEGS
from flygym_amd.controllers import TRIPOD_PHASE_BIAS

BIAS = np.array([TRIPOD_PHASE_BIAS[leg] for leg in LEGS])            # radians
SIDE = np.array([0 if leg[0] == "l" else 1 for leg in LEGS])


def reset_phases(n_worlds, first_world=0, total_worlds=None):
    """(n_worlds, 6) float64: theta_l = (global world / total + b_l / 2 pi) mod 1."""
    w = (first_world + np.arange(n_worlds, dtype=np.float64)) / float(total_worlds or n_worlds)
    return np.mod(w[:, None] + BIAS[None, :] / (2 * np.pi), 1.0)


def wrap(x):
    """Phase difference folded to [-0.5, 0.5) cycles."""
    return np.mod(np.asarray(x, dtype=np.float64) + 0.5, 1.0) - 0.5


def rollout(cycle, leg_of_col, phase, magnitude, drive, n_steps, *, timestep, frequency=12.0, coupling=10.0, convergence=20.0,
            stance=None, adhesion=(1.0, 0.0), dtype=np.float64):
    """``n_steps`` steps of n worlds from ``phase`` (n, 6), ``magnitude`` (n, 6) under the constant ``drive`` (n, 2).

    Returns ``(rows, phases, magnitudes, phase_end, magnitude_end)``: ``rows`` (n, n_steps, n_pos [+ 6]) in ``dtype``,
    ``phases`` (n, n_steps, 6) float64 and ``magnitudes`` (n, n_steps, 6) ``dtype`` — the state each row was computed from — and
    the state after the last step."""
    f = dtype
    cyc = np.asarray(cycle, dtype=np.float32).astype(f)
    n_bins, n_pos = cyc.shape
    mean = np.asarray(cycle, dtype=np.float64).mean(axis=0).astype(np.float32 if f == np.float32 else f).astype(f)
    lod = np.asarray(leg_of_col)
    th = np.array(phase, dtype=np.float64)
    r = np.array(magnitude, dtype=f)
    n = th.shape[0]
    d = np.asarray(drive, dtype=np.float32).astype(f)[:, SIDE]                                   # (n, 6)
    R, nu = np.abs(d), np.float64(frequency) * np.sign(d).astype(np.float64)
    phi = (BIAS[None, :] - BIAS[:, None]).astype(f)                                                # phi[l, j] = b_j - b_l
    off_diag = ~np.eye(6, dtype=bool)
    n_act = n_pos + (6 if stance is not None else 0)
    rows = np.zeros((n, n_steps, n_act), dtype=f)
    phases, mags = np.zeros((n, n_steps, 6)), np.zeros((n, n_steps, 6), dtype=f)
    cols = np.arange(n_pos)[None, :]
    rate = f(f(timestep) * f(convergence))
    for s in range(n_steps):
        phases[:, s], mags[:, s] = th, r
        x = th * np.float64(n_bins)
        i0 = np.floor(x).astype(np.int64) % n_bins
        fr = (x - np.floor(x)).astype(f)
        i0c, frc = i0[:, lod], fr[:, lod]
        c = ((f(1) - frc) * cyc[i0c, cols] + frc * cyc[(i0c + 1) % n_bins, cols]).astype(f)
        rows[:, s, :n_pos] = c + (r[:, lod] - f(1)) * (c - mean[None, :])
        if stance is not None:
            rows[:, s, n_pos:] = np.where(np.asarray(stance)[i0, np.arange(6)[None, :]], f(adhesion[0]), f(adhesion[1]))
        dth = (th[:, None, :] - th[:, :, None]).astype(f)                                         # [w, l, j] = theta_j - theta_l
        term = (r[:, None, :] * f(coupling) * np.sin((f(2 * np.pi) * dth - phi[None]).astype(f))).astype(f)
        S = np.where(off_diag[None], term, f(0)).sum(axis=2, dtype=f)
        th = th + np.float64(timestep) * (nu + S.astype(np.float64) / (2 * np.pi))
        th = th - np.floor(th)
        th[th >= 1.0] = 0.0
        r = (r + rate * (R - r)).astype(f)
    return rows, phases, mags, th, r
