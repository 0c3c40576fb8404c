"""Motion vision in numpy: the specification of ``flygym_amd/csrc/nmf_motion.hip`` (``sensors.MotionDetectors``).  TEST
INFRASTRUCTURE.

Build-defined and pinned by nothing: the reference snapshot holds no vision processing.  The form is the textbook one — two
low-pass filters per ommatidium, a Hassenstein-Reichardt correlator per pair of neighbours, wide-field sums per eye, an optomotor
drive from the difference of the two eyes' front-to-back flows; every constant is a parameter.  The statement of the model is
include/nmf.h (``nmf_motion_update``).

:func:`update` is the specification proper: float32 with every operation rounded as written, which numpy's float32 arrays give,
each pair's term rounded to 2^-16 and summed as an integer, each quotient one float64 division of exact operands rounded once to
float32.  ``np.fmax`` / ``np.fmin`` are the kernel's ``fmaxf`` / ``fminf``.  :func:`update64` restates the same rule in float64
without the fixed-point step: what the specification's own rounding is measured against."""
import numpy as np

f32 = np.float32

DEFAULTS = dict(tau_fast=0.035, tau_slow=0.15, gain=320.0, delta=0.8, base=1.0, drive_min=0.2, drive_max=1.2)
MAX_OMMATIDIA, MAX_PAIRS = 1024, 3072
CLAMP, SCALE = 4.0, 65536.0                 # a pair's term: clamped to +-4, resolution 2^-16


def coefficient(dt: float, tau: float) -> np.float32:
    """a = 1 - exp(-dt / tau) in float64, rounded once to float32."""
    return f32(1.0 - np.exp(-np.float64(dt) / np.float64(tau)))


def motion_pairs(centres: np.ndarray, reach: float = 1.25):
    """``(pairs (P, 2) int32, weights (P, 2) float32)``: every pair a < b of ommatidia whose centres are closer than ``reach`` times
    the median nearest-neighbour distance, in ascending (a, b), with the unit vector from a to b.  Written per ommatidium, unlike
    ``Retina.motion_pairs``."""
    c = np.asarray(centres, dtype=np.float64)
    n = c.shape[0]
    if n < 2:
        return np.zeros((0, 2), dtype=np.int32), np.zeros((0, 2), dtype=f32)
    nearest = np.empty(n)
    for a in range(n):
        d = np.hypot(c[:, 0] - c[a, 0], c[:, 1] - c[a, 1])
        d[a] = np.inf
        nearest[a] = d.min()
    limit = reach * np.median(nearest)
    pairs, weights = [], []
    for a in range(n - 1):
        v = c[a + 1:] - c[a]
        d = np.hypot(v[:, 0], v[:, 1])
        for j in np.nonzero(d < limit)[0]:
            pairs.append((a, a + 1 + int(j)))
            weights.append(v[j] / d[j])
    assert len(pairs) <= MAX_PAIRS
    return np.array(pairs, dtype=np.int32).reshape(-1, 2), np.array(weights, dtype=np.float64).reshape(-1, 2).astype(f32)


def new_state(n_worlds: int, n_omm: int, dtype=f32) -> dict:
    """Every world fresh, the filters at zero (as a new handle)."""
    return dict(fast=np.zeros((n_worlds, 2, n_omm), dtype=dtype), slow=np.zeros((n_worlds, 2, n_omm), dtype=dtype),
                fresh=np.ones(n_worlds, dtype=bool))


def reset(state: dict, mask=None) -> None:
    """The worlds of ``mask`` (default all) become fresh; nothing else changes."""
    if mask is None:
        state["fresh"][:] = True
    else:
        state["fresh"][np.asarray(mask) != 0] = True


def _filters(state, omm, a_fast, a_slow, dtype):
    omm = np.asarray(omm, dtype=dtype)
    x = (omm[..., 0] + omm[..., 1]).astype(dtype)
    fresh = state["fresh"][:, None, None]
    fast = np.where(fresh, x, state["fast"]).astype(dtype)
    slow = np.where(fresh, x, state["slow"]).astype(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        fast = (fast + (a_fast * (x - fast).astype(dtype)).astype(dtype)).astype(dtype)
        slow = (slow + (a_slow * (x - slow).astype(dtype)).astype(dtype)).astype(dtype)
        hp = (x - slow).astype(dtype)
    state["fast"], state["slow"] = fast, slow
    state["fresh"] = np.zeros_like(state["fresh"])
    return fast, hp


def optomotor(flow, front, *, base, gain, delta, drive_min, drive_max, **_):
    """flow (n, 2, 2) float32 (H, V per eye) -> ``(rotation (n,), translation (n,), drive (n, 2))`` float32: steps 6 and 7.
    ``base``: a scalar or an ``(n, 2)`` array."""
    flow = np.asarray(flow, dtype=f32)
    H = flow[..., 0]
    ftb = np.where(np.asarray(front, dtype=bool), -H, H).astype(f32)
    rotation = (ftb[..., 0] - ftb[..., 1]).astype(f32)
    translation = (ftb[..., 0] + ftb[..., 1]).astype(f32)
    rotation = np.where(rotation == 0, f32(0), rotation).astype(f32)                # (a zero is +0)
    translation = np.where(translation == 0, f32(0), translation).astype(f32)
    r = (f32(gain) * rotation).astype(f32)
    with np.errstate(invalid="ignore"):
        q = (r.astype(np.float64) / (f32(1) + np.abs(r)).astype(f32).astype(np.float64)).astype(f32)
    d = f32(delta)
    o = np.stack([(f32(1) - (d * np.fmax(q, f32(0))).astype(f32)).astype(f32),
                  (f32(1) - (d * np.fmax(-q, f32(0))).astype(f32)).astype(f32)], axis=-1)
    b = np.broadcast_to(np.asarray(base, dtype=f32), o.shape)
    drive = np.fmin(np.fmax((b * o).astype(f32), f32(drive_min)), f32(drive_max)).astype(f32)
    return rotation, translation, drive


def update(state: dict, omm, pairs, weights, *, dt, front=(1, 0), base=None, **params) -> dict:
    """One update of every world, in place on ``state``: ``dict(sums (n, 2, 2) int32, flow (n, 2, 2), rotation (n,),
    translation (n,), drive (n, 2))`` float32 and ``clamped (n, 2)``, the number of each eye's terms that sit on the clamp.  ``omm``
    (n, 2, n_omm, 2) float32; ``base`` None (the default), a scalar or an (n, 2) array."""
    p = {**DEFAULTS, **params}
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    weights = np.asarray(weights, dtype=f32).reshape(-1, 2)
    P = pairs.shape[0]
    assert P <= MAX_PAIRS and state["fast"].shape[-1] <= MAX_OMMATIDIA
    fast, hp = _filters(state, omm, coefficient(dt, p["tau_fast"]), coefficient(dt, p["tau_slow"]), f32)
    a, b = pairs[:, 0], pairs[:, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        d = ((fast[..., a] * hp[..., b]).astype(f32) - (hp[..., a] * fast[..., b]).astype(f32)).astype(f32)      # (n, 2, P)
        terms, clamped = [], 0
        for c in range(2):
            v = np.fmin(np.fmax((d * weights[:, c]).astype(f32), f32(-CLAMP)), f32(CLAMP)).astype(f32)
            clamped = clamped + (np.abs(v) == f32(CLAMP)).sum(axis=-1)
            terms.append(np.rint((v * f32(SCALE)).astype(f32)).astype(np.int64))
    sums = np.stack([t.sum(axis=-1) for t in terms], axis=-1)                         # (n, 2, 2): Sx, Sy per eye
    assert np.abs(sums).max(initial=0) < 2 ** 30
    flow = (sums.astype(np.float64) / np.float64(SCALE * P)).astype(f32) if P else np.zeros(sums.shape, dtype=f32)
    rotation, translation, drive = optomotor(flow, front, **{**p, "base": p["base"] if base is None else base})
    return dict(sums=sums.astype(np.int32), flow=flow, rotation=rotation, translation=translation, drive=drive,
                clamped=np.asarray(clamped))                                              # (n, 2): terms that sit on the clamp


def update64(state: dict, omm, pairs, weights, *, dt, **params) -> np.ndarray:
    """The same filters, correlators and means in float64 with exact coefficients and no fixed point, in place on ``state`` (of
    :func:`new_state` with ``dtype=np.float64``): flow (n, 2, 2) float64."""
    p = {**DEFAULTS, **params}
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    w = np.asarray(weights, dtype=np.float64).reshape(-1, 2)
    fast, hp = _filters(state, omm, -np.expm1(-dt / p["tau_fast"]), -np.expm1(-dt / p["tau_slow"]), np.float64)
    a, b = pairs[:, 0], pairs[:, 1]
    d = fast[..., a] * hp[..., b] - hp[..., a] * fast[..., b]
    if pairs.shape[0] == 0:
        return np.zeros(d.shape[:-1] + (2,))
    return np.stack([(np.clip(d * w[:, 0], -CLAMP, CLAMP)).mean(axis=-1), (np.clip(d * w[:, 1], -CLAMP, CLAMP)).mean(axis=-1)], axis=-1)
