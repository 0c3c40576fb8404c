"""The advected odor plume's specification in numpy (the kernels are ``flygym_amd/csrc/nmf_plume.hip``, the class
``flygym_amd.sensors.OdorPlume``).

Written from the definition, one tick at a time.  A plume is a concentration grid ``c[H, W]`` over the ground plane: cell ``(j, i)``
is centred at ``(x0 + (i + 1/2) h, y0 + (j + 1/2) h)``, and cells outside the grid read as 0 everywhere (clean air in, odor out).
One tick, every cell from the old grid::

    v = w + eddy_gain * E[j, i]                                   (w: the plume's wind; E: optional static eddies)
    d = vx * r;  k = floor(d);  f = d - k;  (l, g) likewise from vy           (r = dt / h: index units, no CFL clamp)
    adv = (1 - g) * ((1 - f) * c[j-l, i-k] + f * c[j-l, i-k-1]) + g * ((1 - f) * c[j-l-1, i-k] + f * c[j-l-1, i-k-1])
    dif = D * ((c[j, i-1] + c[j, i+1]) + (c[j-1, i] + c[j+1, i]) - 4 * c[j, i])                    (D = kappa dt / h^2)
    c_new = max(adv + dif, S)

then per plume ``w <- (w + a * (mean - w)) + b * xi`` with the counter-based noise of :func:`noise`, and ``tick <- tick + 1``.
A reading at ``(x, y)`` is the grid interpolated bilinearly between cell centres at ``u = (x - x0) / h - 1/2``, ``v`` likewise,
times ``scale``; ``u`` outside ``[-1/2, W - 1/2]`` or ``v`` outside ``[-1/2, H - 1/2]`` sets the world's out-of-bounds flag.

``r``, ``D``, ``a`` and ``b`` are float32 numbers (:func:`constants` rounds them once, as the library does); ``dtype`` picks the
arithmetic: ``np.float64`` everything in float64, ``np.float32`` the kernels' flavour, every operation rounded to float32 in the
order written above (the kernels may contract a product into the following sum, which the float32 flavour does not).
"""
import numpy as np

MAX_SHIFT = 4096.0          # whole-cell displacements are clamped here before they become integers (the grid is at most 1024 wide)


def constants(cell_size, tick_s, diffusivity, wind_tau, wind_sigma):
    """``(r, D, a, b)`` = ``(dt / h, kappa dt / h^2, dt / tau, sigma sqrt(dt))``: float64 arithmetic on the float32 parameters,
    rounded to float32 once."""
    h, dt, kappa, tau, sigma = (np.float64(np.float32(v)) for v in (cell_size, tick_s, diffusivity, wind_tau, wind_sigma))
    return np.float32(dt / h), np.float32(kappa * dt / (h * h)), np.float32(dt / tau), np.float32(sigma * np.sqrt(dt))


def hash32(x):
    """The 32-bit mixer, on uint32 arrays."""
    x = np.asarray(x, dtype=np.uint64) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x.astype(np.uint32)


def uniforms(seed, world, tick, m):
    """``hash(seed ^ world * 0x9E3779B9 ^ tick * 0x85EBCA6B ^ m * 0xC2B2AE35) >> 8`` as integers in [0, 2^24) (uint32 arithmetic)."""
    world, tick, m = (np.asarray(v, dtype=np.uint64) for v in (world, tick, m))
    key = (np.uint64(int(seed) & 0xFFFFFFFF) ^ ((world * 0x9E3779B9) & 0xFFFFFFFF) ^ ((tick * 0x85EBCA6B) & 0xFFFFFFFF)
           ^ ((m * 0xC2B2AE35) & 0xFFFFFFFF))
    return hash32(key) >> 8


def noise(seed, world, tick, m0, dtype=np.float64):
    """``xi = ((u0 + u1) + (u2 + u3) - 2) * sqrt(3)`` with ``u_m = uniforms(.., m0 + m) * 2^-24``: mean 0, variance 1."""
    f = dtype
    u = [uniforms(seed, world, tick, m0 + m).astype(f) * f(2.0 ** -24) for m in range(4)]
    return (((u[0] + u[1]) + (u[2] + u[3])) - f(2)) * f(np.sqrt(3.0))


def _cell(c, jj, ii):
    """``c[jj, ii]``, 0 outside the grid."""
    H, W = c.shape
    inside = (jj >= 0) & (jj < H) & (ii >= 0) & (ii < W)
    return np.where(inside, c[np.clip(jj, 0, H - 1), np.clip(ii, 0, W - 1)], c.dtype.type(0))


def _blend(c, jj, ii, dj, di, g, f):
    one = c.dtype.type(1)
    return ((one - g) * ((one - f) * _cell(c, jj, ii) + f * _cell(c, jj, ii + di))
            + g * ((one - f) * _cell(c, jj + dj, ii) + f * _cell(c, jj + dj, ii + di)))


def _floor_int(d):
    return np.clip(np.floor(d), -MAX_SHIFT, MAX_SHIFT).astype(np.int64)


def tick(c, wind, *, r, D, source, eddies=None, eddy_gain=0.0, dtype=np.float64):
    """One grid update of ``c`` ``(n, H, W)`` under the winds ``(n, 2)``; returns the new grids in ``dtype``."""
    f = dtype
    c = np.asarray(c).astype(f)
    wind = np.asarray(wind).astype(f)
    S = np.asarray(source, dtype=np.float32).astype(f)
    n, H, W = c.shape
    jj, ii = np.mgrid[0:H, 0:W]
    out = np.empty_like(c)
    for p in range(n):
        vx, vy = np.full((H, W), wind[p, 0], dtype=f), np.full((H, W), wind[p, 1], dtype=f)
        if eddies is not None:
            E = np.asarray(eddies, dtype=np.float32).astype(f)
            vx, vy = vx + f(eddy_gain) * E[..., 0], vy + f(eddy_gain) * E[..., 1]
        dx, dy = vx * f(r), vy * f(r)
        k, l = _floor_int(dx), _floor_int(dy)
        adv = _blend(c[p], jj - l, ii - k, -1, -1, dy - np.floor(dy), dx - np.floor(dx))
        ring = (_cell(c[p], jj, ii - 1) + _cell(c[p], jj, ii + 1)) + (_cell(c[p], jj - 1, ii) + _cell(c[p], jj + 1, ii))
        out[p] = np.maximum(adv + f(D) * (ring - f(4) * c[p]), S)
    return out


def wind_step(wind, ticks, *, a, b, mean, seed, first_world=0, dtype=np.float64):
    """The Ornstein-Uhlenbeck step of the winds ``(n, 2)`` at the tick counters ``ticks`` ``(n,)`` (their values BEFORE the
    increment); returns the new winds in ``dtype``."""
    f = dtype
    w = np.asarray(wind).astype(f)
    world = first_world + np.arange(w.shape[0])
    mean = np.asarray(mean, dtype=np.float32).astype(f)
    xi = np.stack([noise(seed, world, ticks, 0, f), noise(seed, world, ticks, 4, f)], axis=1)
    return ((w + f(a) * (mean[None, :] - w)) + f(b) * xi).astype(f)


def advance(c, wind, ticks, n_ticks, *, r, D, a, b, mean, seed, source, eddies=None, eddy_gain=0.0, first_world=0, dtype=np.float64):
    """``n_ticks`` ticks; returns ``(c, wind, ticks, winds)`` with ``winds`` ``(n_ticks, n, 2)`` the wind after every tick."""
    ticks = np.array(ticks, dtype=np.int64)
    winds = []
    for _ in range(n_ticks):
        c = tick(c, wind, r=r, D=D, source=source, eddies=eddies, eddy_gain=eddy_gain, dtype=dtype)
        wind = wind_step(wind, ticks, a=a, b=b, mean=mean, seed=seed, first_world=first_world, dtype=dtype)
        ticks = ticks + 1
        winds.append(wind)
    return c, wind, ticks, np.stack(winds)


def read(c, points, *, cell_size, origin, scale=1.0, dtype=np.float64):
    """Readings of the grids ``c`` ``(n, H, W)`` (or one shared grid ``(1, H, W)``) at ``points`` ``(n_worlds, n_pts, 2)``:
    ``(values (n_worlds, n_pts) in dtype, flags (n_worlds,) uint8)``."""
    f = dtype
    c = np.asarray(c).astype(f)
    pts = np.asarray(points, dtype=np.float32).astype(f)
    h, x0, y0 = (f(np.float32(v)) for v in (cell_size, origin[0], origin[1]))
    _, H, W = c.shape
    u = ((pts[..., 0] - x0) / h - f(0.5)).astype(f)
    v = ((pts[..., 1] - y0) / h - f(0.5)).astype(f)
    oob = ~((u >= -0.5) & (u <= W - 0.5) & (v >= -0.5) & (v <= H - 0.5))
    near = (u > -1) & (u < W) & (v > -1) & (v < H)                     # else all four cells lie outside
    uu, vv = np.where(near, u, f(0)), np.where(near, v, f(0))
    out = np.zeros(u.shape, dtype=f)
    for w in range(pts.shape[0]):
        g = c[0 if c.shape[0] == 1 else w]
        i0, j0 = np.floor(uu[w]).astype(np.int64), np.floor(vv[w]).astype(np.int64)
        val = _blend(g, j0, i0, 1, 1, vv[w] - np.floor(vv[w]), uu[w] - np.floor(uu[w])) * f(np.float32(scale))
        out[w] = np.where(near[w], val, f(0))
    return out, oob.any(axis=1).astype(np.uint8)
