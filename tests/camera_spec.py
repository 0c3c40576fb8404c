"""The batch camera renderer's specification in numpy (the kernel is ``flygym_amd/csrc/nmf_camera.hip``).

Written from the definition, not from the kernel: every pixel is tested against every object, no culling, in the float type
given (float64 by default; float32 to measure what the number format alone does to a frame).

* camera: pinhole; pixel (row, col) of an H x W image has the camera-frame ray ``(u, -v, -1)`` normalised,
  ``u = (col + 0.5 - W/2) t``, ``v = (row + 0.5 - H/2) t``, ``t = tan(fovy/2) / (H/2)``; x right, y up, the camera looks along
  -z; ``cam_mat`` has the right / up / back axes in its columns;
* scene: ``flygym_amd.vision.Scene`` — checker ground z = ground_z (parity of floor(x/s) + floor(y/s)) or, with a terrain,
  the relief the physics collides with: constant-height cells of h(x, y) followed cell by cell for at most
  ``MAX_TERRAIN_CELLS`` cells, side walls included, the flat plane's answer beyond; a uniform sky; opaque spheres; capsules
  (end points in world coordinates, radius), each with a colour; the nearest positive hit wins;
* shading: ``colour = base * (ambient + diffuse * max(0, n_z))`` with the hit's unit surface normal n (ground and block tops
  n_z = 1, side walls n_z = 0), rounded as ``floor(x + 0.5)`` and clipped to uint8; the sky is not a surface and keeps its colour.

Besides the colours, each pixel's hit id is returned: ``SKY``, ``GROUND_A`` / ``GROUND_B`` (the two checker colours — finer than
"ground", so that a pixel on the other side of a checker edge counts as another hit instead of as a colour error), ``WALL``,
``SPHERE0 + i``, ``CAPSULE0 + k``.
"""
import numpy as np

from sensors_oracle import MAX_TERRAIN_CELLS, TERRAIN_EPS, TERRAIN_WALL_TOL

SKY, GROUND_A, GROUND_B, WALL, SPHERE0, CAPSULE0 = 0, 1, 2, 3, 16, 64


def pixel_rays(height, width, fovy_deg, f=np.float64):
    """Camera-frame unit rays (H, W, 3)."""
    t = f(np.tan(0.5 * np.deg2rad(float(fovy_deg))) / (0.5 * height))
    i, j = np.mgrid[0:height, 0:width]
    u = ((j.astype(f) + f(0.5) - f(0.5 * width)) * t).astype(f)
    v = ((i.astype(f) + f(0.5) - f(0.5 * height)) * t).astype(f)
    n = np.sqrt(u * u + v * v + f(1)).astype(f)
    return np.stack([u / n, -v / n, -f(1) / n], axis=-1).astype(f)


def terrain_cell(kind, p, x, y, f=np.float64):
    """(x0, x1, y0, y1, h) of the constant-height cell of the build-defined terrains (flygym_amd/compose/world.py) that holds
    (x, y) — ``oracle/sensors_oracle.py::terrain_cell`` in the float type ``f``."""
    x, y = np.asarray(x, dtype=f), np.asarray(y, dtype=f)
    inf = np.full(x.shape, np.inf, dtype=f)

    def gapped(block, gap, depth):
        period = f(f(block) + f(gap))
        base = (np.floor(x / period) * period).astype(f)
        on = (x - base) < f(block)
        return (np.where(on, base, base + f(block)).astype(f), np.where(on, base + f(block), base + period).astype(f), -inf, inf,
                np.where(on, f(0), f(-depth)).astype(f))

    def blocks(size, height):
        i, j = np.floor(x / f(size)).astype(f), np.floor(y / f(size)).astype(f)
        ssum = i + j
        par = ssum - f(2) * np.floor(ssum / f(2))
        return ((i * f(size)).astype(f), ((i + 1) * f(size)).astype(f), (j * f(size)).astype(f), ((j + 1) * f(size)).astype(f),
                np.where(par != 0, f(height), f(0)).astype(f))

    if kind == 1:
        return gapped(p[0], p[1], p[2])
    if kind == 2:
        return blocks(p[0], p[1])
    if kind == 3:
        st = np.floor(x / f(p[3])).astype(f)
        k = st - f(3) * np.floor(st / f(3))
        s0, s1 = (st * f(p[3])).astype(f), ((st + 1) * f(p[3])).astype(f)
        g, bk = gapped(1.0, p[1], p[2]), blocks(p[0], 0.35)
        x0 = np.where(k == 1, np.maximum(g[0], s0), np.where(k == 2, np.maximum(bk[0], s0), s0)).astype(f)
        x1 = np.where(k == 1, np.minimum(g[1], s1), np.where(k == 2, np.minimum(bk[1], s1), s1)).astype(f)
        y0 = np.where(k == 2, bk[2], -inf).astype(f)
        y1 = np.where(k == 2, bk[3], inf).astype(f)
        h = np.where(k == 1, g[4], np.where(k == 2, bk[4], f(0))).astype(f)
        return x0, x1, y0, y1, h
    return -inf, inf, -inf, inf, np.zeros(x.shape, dtype=f)


def ray_capsule(d, pa, pb, r, f=np.float64):
    """Nearest positive hit of unit rays d (.., 3) from the origin with the capsule (pa, pb, r): ``(t, n_z)``; t = inf: miss.
    The side is the cylinder about the axis between the end points, the ends are the spheres at pa and pb."""
    pa, pb, r = np.asarray(pa, dtype=f), np.asarray(pb, dtype=f), f(r)
    ba = pb - pa
    baba, baoa, oaoa = ba @ ba, -(ba @ pa), pa @ pa
    bard, rdoa = d @ ba, -(d @ pa)
    a = baba - bard * bard
    b = baba * rdoa - baoa * bard
    c = baba * oaoa - baoa * baoa - r * r * baba
    h = b * b - a * c
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (-b - np.sqrt(np.maximum(h, 0))) / a
    yy = baoa + t * bard
    cyl = (h >= 0) & (a > f(1e-12))
    side = cyl & (yy > 0) & (yy < baba) & (t > 0)
    use_a = ~(yy > 0) | ~cyl
    centre = np.where(use_a[..., None], pa, pb)
    bb = -(d * centre).sum(axis=-1)
    hh = bb * bb - ((centre * centre).sum(axis=-1) - r * r)
    with np.errstate(invalid="ignore"):
        te = -bb - np.sqrt(np.maximum(hh, 0))
    end = (hh > 0) & (te > 0)
    t_hit = np.where(side, t, np.where(end, te, np.inf)).astype(f)
    with np.errstate(invalid="ignore", over="ignore"):
        z_axis = np.where(side, pa[2] + ba[2] * (yy / baba), centre[..., 2])
        nz = np.where(np.isfinite(t_hit), (t_hit * d[..., 2] - z_axis) / r, 0)
    return t_hit, nz.astype(f)


def render(cam_pos, cam_mat, height, width, fovy_deg, *, checker_size=4.0, ground_z=0.0, sky_rgb=(140, 179, 230),
           ground_rgb=((77, 77, 77), (102, 102, 102)), wall_rgb=(51, 51, 51), spheres=(), sphere_rgb=(), terrain=None,
           capsules=(), capsule_rgb=(), ambient=0.4, diffuse=0.6, dtype=np.float64):
    """One camera's frame: ``(rgb (H, W, 3) uint8, hit id (H, W) int)``.  ``terrain``: None or (kind, parameters p0..p3,
    highest level); ``capsules``: (p0, p1, radius) in world coordinates; colours are uint8 triples."""
    f = dtype
    d = (pixel_rays(height, width, fovy_deg, f) @ np.asarray(cam_mat, dtype=f).T).astype(f)
    cam = np.asarray(cam_pos, dtype=f)
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    hit = np.full((height, width), SKY, dtype=np.int64)
    tbest = np.full((height, width), np.inf, dtype=f)
    nz = np.zeros((height, width), dtype=f)
    inv_cs = f(1.0) / f(checker_size)

    def parity(t, mask):
        with np.errstate(invalid="ignore"):
            qx = np.where(mask, (cam[0] + t * dx) * inv_cs, 0)
            qy = np.where(mask, (cam[1] + t * dy) * inv_cs, 0)
        return (np.floor(qx).astype(np.int64) + np.floor(qy).astype(np.int64)) & 1

    with np.errstate(divide="ignore", invalid="ignore"):
        t = (-(cam[2] - f(ground_z)) / dz).astype(f)
    g = (dz < 0) & (t > 0)
    hit = np.where(g, GROUND_A + parity(t, g), hit)
    tbest = np.where(g, t, tbest)
    nz = np.where(g, f(1), nz)
    if terrain is not None and int(terrain[0]) != 0:
        kind, tp, hmax = int(terrain[0]), [float(v) for v in terrain[1]], f(terrain[2])
        down = dz < 0
        with np.errstate(divide="ignore", invalid="ignore"):
            tcur = np.where(down, np.maximum(f(0), (f(ground_z) + hmax - cam[2]) / dz), np.inf).astype(f)
        live = down.copy()
        t_hit = np.full((height, width), np.inf, dtype=f)
        m_hit = np.zeros((height, width), dtype=np.int64)
        for _ in range(MAX_TERRAIN_CELLS):
            tprobe = tcur + f(TERRAIN_EPS)
            with np.errstate(invalid="ignore"):
                px, py = np.where(live, cam[0] + tprobe * dx, 0), np.where(live, cam[1] + tprobe * dy, 0)
            x0, x1, y0, y1, h = terrain_cell(kind, tp, px, py, f)
            h = h + f(ground_z)
            with np.errstate(divide="ignore", invalid="ignore"):
                z_in = cam[2] + tcur * dz
                wall = live & (z_in < h - f(TERRAIN_WALL_TOL))
                tx = np.where(dx > 0, (x1 - cam[0]) / dx, np.where(dx < 0, (x0 - cam[0]) / dx, np.inf))
                ty = np.where(dy > 0, (y1 - cam[1]) / dy, np.where(dy < 0, (y0 - cam[1]) / dy, np.inf))
                t_h = (h - cam[2]) / dz
            t_out = np.minimum(tx, ty)
            top = live & ~wall & (t_h <= t_out)
            t_hit = np.where(wall, tcur, np.where(top, t_h, t_hit)).astype(f)
            m_hit = np.where(wall, WALL, np.where(top, GROUND_A + parity(t_h, top), m_hit))
            live = live & ~wall & ~top
            tcur = np.where(live, t_out, tcur).astype(f)
        done = down & ~live
        hit = np.where(done, m_hit, hit)
        tbest = np.where(done, t_hit, tbest)
        nz = np.where(done, np.where(m_hit == WALL, f(0), f(1)), nz)
    for s, sp in enumerate(spheres):
        sp = np.asarray(sp, dtype=f)
        oc = cam - sp[:3]
        b = d @ oc
        disc = b * b - (oc @ oc - sp[3] * sp[3])
        with np.errstate(invalid="ignore"):
            ts = -b - np.sqrt(np.maximum(disc, 0))
        ok = (disc > 0) & (ts > 0) & (ts < tbest)
        hit = np.where(ok, SPHERE0 + s, hit)
        nz = np.where(ok, (oc[2] + ts * dz) / sp[3], nz)
        tbest = np.where(ok, ts, tbest).astype(f)
    for k, cap in enumerate(capsules):
        tc, nzc = ray_capsule(d, np.asarray(cap[0], dtype=f) - cam, np.asarray(cap[1], dtype=f) - cam, cap[2], f)
        ok = tc < tbest
        hit = np.where(ok, CAPSULE0 + k, hit)
        nz = np.where(ok, nzc, nz)
        tbest = np.where(ok, tc, tbest).astype(f)
    # colours
    n_obj = max(CAPSULE0 + len(capsules), SPHERE0 + 8)
    palette = np.zeros((n_obj, 3), dtype=f)
    palette[SKY], palette[GROUND_A], palette[GROUND_B], palette[WALL] = sky_rgb, ground_rgb[0], ground_rgb[1], wall_rgb
    for s, c in enumerate(sphere_rgb):
        palette[SPHERE0 + s] = c
    for k in range(len(capsules)):
        palette[CAPSULE0 + k] = capsule_rgb[k]
    factor = np.where(hit == SKY, f(1), f(ambient) + f(diffuse) * np.maximum(nz, f(0))).astype(f)
    rgb = np.clip(np.floor(palette[hit] * factor[..., None] + f(0.5)), 0, 255).astype(np.uint8)
    return rgb, hit


def world_capsules(seg_xpos, seg_xquat, cap_seg, cap_geom):
    """(p0, p1, radius) in world coordinates of capsules given in their segments' frames; poses of one world, float64."""
    from sensors_oracle import quat_to_mat

    out = []
    for sg, g in zip(cap_seg, np.asarray(cap_geom, dtype=np.float64)):
        R, p = quat_to_mat(np.asarray(seg_xquat[sg], dtype=np.float64)), np.asarray(seg_xpos[sg], dtype=np.float64)
        out.append((p + R @ g[:3], p + R @ g[3:6], float(g[6])))
    return out
