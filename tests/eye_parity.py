"""What the eye renderer's parity tests share (tests/test_eye_oracle_cpu.py, tests/test_eye_parity_gpu.py): the interior rule,
the scenes of the float32 / float64 comparison of the specification, the lens rule of the visit plan and small retinas.
TEST INFRASTRUCTURE; needs no GPU."""
import numpy as np

import sensors_oracle as so

SKY, GROUND, WALL, BODY = (140, 178, 230), ((77, 77, 77), (102, 102, 102)), (51, 51, 51), (120, 90, 60)
TERRAINS = {0: None, 1: (1, (1.0, 0.3, 2.0, 0.0), 0.0), 2: (2, (1.3, 0.35, 0.0, 0.0), 0.35), 3: (3, (1.3, 0.3, 2.0, 4.0), 0.35)}


SMALL_RETINAS = {(48, 64): (6, 8), (64, 50): (9, 7), (80, 96): (9, 11)}      # (height, width): lattice rows x cols (48, 63 and 99 ommatidia)
# (lens polynomials serve the frame, pixels behind the fisheye's full sphere) by the visit plan's rule, nmf_capi.hip `lens_ok`: every
# pixel's polar angle below 2.1 rad.  The corners of a 64- or 96-wide retina lie at rho = 1.64 / 1.54, so 157 degrees is the
# polynomial path on the 50-wide one only: 140 degrees is here to run that path at the two widths where no chunk wraps.
LENS_PATHS = {(48, 64): {140: (True, 0), 157: (False, 0), 250: (False, 136), 300: (False, 672)},
        (64, 50): {140: (True, 0), 157: (True, 0), 250: (False, 0), 300: (False, 20)},
        (80, 96): {140: (True, 0), 157: (False, 0), 250: (False, 96), 300: (False, 1024)}}


def interior_mask(mat: np.ndarray) -> np.ndarray:
    """A pixel is interior if the material image has its value on the pixel's whole 3 x 3 neighbourhood (pixels on the image
    border: the neighbours that exist)."""
    h, w = mat.shape
    pad = np.pad(mat, 1, mode="edge")           # (a border pixel's missing neighbours repeat existing ones)
    same = np.ones((h, w), dtype=bool)
    for di in (0, 1, 2):
        for dj in (0, 1, 2):
            same &= pad[di:di + h, dj:dj + w] == mat
    return same


def known_answer_scenes():
    """Every call of the two known-answer tests of tests/test_sensors.py (test_eye_render_oracle_*), as (args, kwargs)."""
    H, W, fov = 512, 450, 157.0
    down = np.eye(3)
    gapped, blocks = TERRAINS[1], TERRAINS[2]
    base = lambda pos, cs=4.0: (pos, down, H, W, fov, cs, 0.0, SKY, GROUND)
    return [
        (base((0.5, 0.5, 2.0)), {}),
        (base((0.5, 0.5, 2.0)) + ([(0.5, 0.5, 1.0, 0.4)], [(10, 20, 30)]), {}),
        (base((0.5, 0.5, 2.0)), dict(terrain=gapped, wall_rgb=WALL)),
        (base((1.15, 0.5, 2.0)), dict(terrain=gapped, wall_rgb=WALL)),
        (base((1.3, 1.3, 2.0), 100.0), dict(terrain=blocks, wall_rgb=WALL)),
        (base((0.5, 0.5, 2.0)), dict(capsules=[((0.2, 0.5, 1.0), (0.8, 0.5, 1.0), 0.1)], body_rgb=BODY)),
        (base((0.5, 0.5, 2.0)), dict(capsules=[((0.2, 0.5, -1.0), (0.8, 0.5, -1.0), 0.1)], body_rgb=BODY)),
    ]


def synthetic_scene(kind: int, seed: int):
    """A scene like an eye's: terrain ``kind``, a camera 1.0 to 1.8 mm up that looks as the left eye does (with jitter), 54 or 55
    capsules of radius 0.02 to 0.12 mm within about 1 mm of it, two spheres; 512 x 450 pixels at 157 degrees."""
    rng = np.random.default_rng(1000 * kind + seed)
    cam = np.array([rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(1.0, 1.8)])
    R = so.euler_xyz_extrinsic_to_mat((1.57 + rng.normal(0, 0.15), rng.normal(0, 0.15), -0.47 + rng.normal(0, 0.3)))
    caps = []
    for _ in range(54 + int(rng.integers(0, 2))):
        p0 = cam + rng.normal(0, 0.6, 3)
        p0[2] = max(p0[2], 0.1)
        if np.linalg.norm(p0 - cam) < 0.25:
            p0 = cam + (p0 - cam) * 0.25 / max(np.linalg.norm(p0 - cam), 1e-6)
        p1 = p0 + rng.normal(0, 0.25, 3)
        caps.append((p0, p1, float(rng.uniform(0.02, 0.12))))
    spheres = [(cam[0] + 6.0, cam[1] + 4.0, 1.5, 1.0), (cam[0] - 2.0, cam[1] + 5.0, 0.8, 0.8)]
    args = (cam, R, 512, 450, 157.0, 4.0, 0.0, SKY, GROUND, spheres, [(230, 51, 26), (13, 13, 13)])
    return args, dict(terrain=TERRAINS[kind], wall_rgb=WALL, capsules=caps, body_rgb=BODY)


def lens_path(height: int, width: int, fov_deg: float):
    """(lens_ok, n_black): the visit plan's rule (csrc/nmf_capi.hip, ``cones[..][9]``) — the kernel's lens polynomials serve a frame
    whose every pixel has a polar angle below 2.1 rad — and the number of pixels behind the fisheye's full sphere."""
    i, j = np.mgrid[0:height, 0:width]
    u, v = (j + 0.5 - 0.5 * width) * 2.0 / height, (i + 0.5 - 0.5 * height) * 2.0 / height
    theta = np.sqrt(np.maximum(u * u + v * v, 1e-24)) * (0.5 * fov_deg * np.pi / 180.0)
    return bool((-np.cos(theta) < -np.cos(2.1)).all()), int((theta > np.pi).sum())


def lattice_id_map(height: int, width: int, rows: int, cols: int, border: int = 2, seed: int = 0) -> np.ndarray:
    """(height, width) int16 id map of rows x cols rectangular cells of unequal size inside a background border."""
    rng = np.random.default_rng(seed)

    def cuts(lo, hi, n):
        inner = np.sort(rng.choice(np.arange(lo + 2, hi - 1), size=n - 1, replace=False))
        return np.concatenate([[lo], inner, [hi]])

    rc, cc = cuts(border, height - border, rows), cuts(border, width - border, cols)
    out = np.zeros((height, width), dtype=np.int16)
    for a in range(rows):
        for b in range(cols):
            out[rc[a]:rc[a + 1], cc[b]:cc[b + 1]] = 1 + a * cols + b
    return out


def check_known_answers(render=so.render_eye_frames):
    """The flat scene of the renderer's specification against geometry worked by hand; ``render``: a flavour of
    sensors_oracle.render_eye_frames."""
    H, W, fov, h = 512, 450, 157.0, 2.0
    sky, ground = (140, 178, 230), ((77, 77, 77), (102, 102, 102))
    down = np.eye(3)                                                    # camera axes = world axes: looks along -z (down)
    fr = render((0.5, 0.5, h), down, H, W, fov, 4.0, 0.0, sky, ground)
    assert fr.shape == (H, W, 3) and fr.dtype == np.uint8
    # straight below (0.5, 0.5): square (0, 0) -> parity 0 -> colour A; the image centre is between 4 pixels
    assert (fr[255:257, 224:226] == ground[0]).all()
    # along the middle row a pixel at rho sees the ground at x = 0.5 + h tan(rho * fov / 2): check a few columns
    for col in (260, 300, 330, 360, 400):
        rho = (col + 0.5 - W / 2) * 2 / H
        x = 0.5 + h * np.tan(rho * np.radians(fov / 2))
        want = ground[(int(np.floor(x / 4.0)) + 0) & 1]
        if abs(x / 4.0 - round(x / 4.0)) > 1e-3:                         # not on a checker edge
            assert tuple(fr[256, col]) == want, col
    # the horizon is at rho = 90 / 78.5 > 1 along the axes but inside the corners: sky only there
    rho_corner = np.hypot(W / H, 1.0)
    assert rho_corner * fov / 2 > 90
    assert tuple(fr[0, 0]) == sky and tuple(fr[0, W // 2]) != sky
    # a sphere right below: angular radius asin(r / d) -> a disc of that many pixels
    fr2 = render((0.5, 0.5, h), down, H, W, fov, 4.0, 0.0, sky, ground, [(0.5, 0.5, 1.0, 0.4)], [(10, 20, 30)])
    n_sphere = int((fr2 == (10, 20, 30)).all(axis=-1).sum())
    r_pix = np.arcsin(0.4 / 1.0) / np.radians(fov / 2) * H / 2
    assert abs(n_sphere - np.pi * r_pix ** 2) < 0.03 * np.pi * r_pix ** 2
    # the legacy eye orientations, read as extrinsic x-y-z rotations, look forward-sideways with +z up
    L = so.euler_xyz_extrinsic_to_mat((1.57, 0.0, -0.47))
    Rr = so.euler_xyz_extrinsic_to_mat((-1.57, 3.14, 0.47))
    np.testing.assert_allclose(L @ [0, 0, -1], [np.sin(0.47), np.cos(0.47), 0], atol=2e-3)
    np.testing.assert_allclose(Rr @ [0, 0, -1], [np.sin(0.47), -np.cos(0.47), 0], atol=2e-3)
    assert (L @ [0, 1, 0])[2] > 0.999 and (Rr @ [0, 1, 0])[2] > 0.999


def check_terrain_and_body_known_answers(render=so.render_eye_frames):
    """The relief and body parts of the renderer's specification against geometry worked by hand."""
    H, W, fov = 512, 450, 157.0
    sky, ground, wall, body = (140, 178, 230), ((77, 77, 77), (102, 102, 102)), (51, 51, 51), (120, 90, 60)
    down = np.eye(3)
    gapped = (1, (1.0, 0.3, 2.0, 0.0), 0.0)
    # straight above the middle of a 1 mm block (x = 0.5): the centre pixels see its top, i.e. the flat answer
    flat = render((0.5, 0.5, 2.0), down, H, W, fov, 4.0, 0.0, sky, ground)
    fr = render((0.5, 0.5, 2.0), down, H, W, fov, 4.0, 0.0, sky, ground, terrain=gapped, wall_rgb=wall)
    assert (fr[250:262, 219:231] == flat[250:262, 219:231]).all()
    # straight above the middle of a gap (x = 1.15, 2 mm deep, 0.3 mm wide): the centre sees the gap floor (a top surface,
    # checker colour), a ray that leaves the gap sideways before reaching the floor sees a wall
    fr = render((1.15, 0.5, 2.0), down, H, W, fov, 4.0, 0.0, sky, ground, terrain=gapped, wall_rgb=wall)
    assert tuple(fr[256, 225]) in ground
    # along the middle row (varying x): the ray with tan(angle) = 0.15 / 4 just reaches the floor's edge; beyond it -> wall
    ang_edge = np.arctan(0.15 / 4.0)
    col_edge = W / 2 + ang_edge / np.radians(fov / 2) * H / 2
    assert tuple(fr[256, int(col_edge) + 3]) == wall and tuple(fr[256, int(col_edge) - 3]) in ground
    # walls are seen only on the relief
    assert not (flat == wall).all(axis=-1).any() and (fr == wall).all(axis=-1).mean() > 0.05
    # blocks: above the corner of four squares each quadrant of the centre shows tops at two different levels -> the raised
    # squares look larger (closer): count of raised-top pixels > count of low-top pixels near the centre
    blocks = (2, (1.3, 0.35, 0.0, 0.0), 0.35)
    frb = render((1.3, 1.3, 2.0), down, H, W, fov, 100.0, 0.0, sky, ground, terrain=blocks, wall_rgb=wall)
    assert (frb == wall).all(axis=-1).any()
    # a capsule along x right below the camera: its silhouette is about (length + 2 r) x 2 r at distance 1
    cap = [((0.2, 0.5, 1.0), (0.8, 0.5, 1.0), 0.1)]
    frc = render((0.5, 0.5, 2.0), down, H, W, fov, 4.0, 0.0, sky, ground, capsules=cap, body_rgb=body)
    mask = (frc == body).all(axis=-1)
    px_per_rad = H / 2 / np.radians(fov / 2)
    want = (2 * np.arctan(0.3 / 0.9)) * (2 * np.arcsin(0.1 / 1.0)) * px_per_rad ** 2
    assert 0.75 * want < mask.sum() < 1.15 * want
    rows, cols = np.where(mask)
    assert abs(rows.mean() - 255.5) < 1.0 and abs(cols.mean() - 224.5) < 1.0 and np.ptp(cols) > 2.5 * np.ptp(rows)
    # nearest hit wins: a capsule below the ground plane is hidden
    hidden = render((0.5, 0.5, 2.0), down, H, W, fov, 4.0, 0.0, sky, ground, capsules=[((0.2, 0.5, -1.0), (0.8, 0.5, -1.0), 0.1)], body_rgb=body)
    assert (hidden == flat).all()


# ---- the parity rule of tests/test_eye_parity_gpu.py: colours that name the material, the float64 view of a pose
# (every green and blue byte differs from material to material, so a reading moves with any pixel; none exceeds 250, which leaves
# the reading bound (differing pixels) / (pixels) a fiftieth of slack over float32 rounding)
PALETTE = {"sky": (10, 200, 220), "ground": ((20, 60, 80), (30, 100, 120)), "wall": (40, 30, 45), "body": (50, 150, 20),
           "spheres": tuple((60 + 10 * s, 240 - 25 * s, 15 + 28 * s) for s in range(8))}


def palette_materials(n_spheres: int) -> dict:
    """{packed rgb: material} for 0 sky, 1 / 2 ground, 3 wall, 4 body, 5.. spheres, -1 black."""
    cols = [PALETTE["sky"], *PALETTE["ground"], PALETTE["wall"], PALETTE["body"], *PALETTE["spheres"][:n_spheres]]
    table = {(c[0] << 16) | (c[1] << 8) | c[2]: m for m, c in enumerate(cols)}
    table[0] = -1
    assert len(table) == 6 + n_spheres
    return table


def decode_materials(frame: np.ndarray, n_spheres: int) -> np.ndarray:
    """The material image a frame drawn with PALETTE names; a colour outside the palette is an error."""
    packed = (frame[..., 0].astype(np.int64) << 16) | (frame[..., 1].astype(np.int64) << 8) | frame[..., 2].astype(np.int64)
    out = np.full(packed.shape, -99, dtype=np.int64)
    for rgb, m in palette_materials(n_spheres).items():
        out[packed == rgb] = m
    assert (out != -99).all(), f"{int((out == -99).sum())} pixels carry a colour no material has"
    return out


def quat_mul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = np.moveaxis(np.asarray(b, dtype=np.float64), -1, 0)
    return np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], axis=-1)


def move_rigidly(xpos, xquat, axis, angle_deg, centre_to, about=0):
    """All segments (nseg, 3) / (nseg, 4) turned by ``angle_deg`` about ``axis`` through segment ``about`` (the thorax), which then
    moves to ``centre_to`` (None entries keep the coordinate).  float64 in, float64 out."""
    xpos, xquat = np.asarray(xpos, dtype=np.float64), np.asarray(xquat, dtype=np.float64)
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    half = np.radians(angle_deg) / 2
    q = np.array([np.cos(half), *(np.sin(half) * axis)])
    c = xpos[about].copy()
    target = np.array([c[i] if v is None else v for i, v in enumerate(centre_to)], dtype=np.float64)
    return (xpos - c) @ so.quat_to_mat(q).T + target, quat_mul(q, xquat)


def eye_camera(xpos, xquat, seg_index, rel_pos, rel_quat):
    """World position and axes (columns right, up, back) of an eye camera attached to segment ``seg_index``."""
    Rs = so.quat_to_mat(xquat[seg_index])
    return xpos[seg_index] + Rs @ np.asarray(rel_pos, dtype=np.float64), Rs @ so.quat_to_mat(rel_quat)


def world_capsules(xpos, xquat, capsule_seg, capsule_geom):
    caps = []
    for sg, g in zip(capsule_seg, np.asarray(capsule_geom, dtype=np.float64)):
        Rm = so.quat_to_mat(xquat[sg])
        caps.append((xpos[sg] + Rm @ g[0:3], xpos[sg] + Rm @ g[3:6], g[6]))
    return caps


def spec_view(cam, R, height, width, fov_deg, terrain, spheres, capsules, dtype, checker_size=4.0):
    """(frame, materials) of the specification in ``dtype``, drawn with PALETTE (ground at z = 0)."""
    return so.render_eye_frames(cam, R, height, width, fov_deg, checker_size, 0.0, PALETTE["sky"], PALETTE["ground"], [tuple(s) for s in spheres],
                                PALETTE["spheres"][:len(spheres)], terrain=terrain, wall_rgb=PALETTE["wall"], capsules=capsules,
                                body_rgb=PALETTE["body"], dtype=dtype, return_materials=True)


def eight_spheres(cams):
    """Eight spheres about a fly whose eye cameras are ``cams`` = [(position, axes)] (left, right): [0] encloses both cameras, [1] and
    [5] sit directly behind the left / the right eye, [2] is cut by the ground plane, [3] and [4] overlap in the left eye's image at
    different depths, [6] is in the right eye's view, [7] is small and far.  float32 (8, 4)."""
    (cl, Rl), (cr, Rr) = cams
    fl, fr, up = -Rl[:, 2], -Rr[:, 2], np.array([0.0, 0.0, 1.0])
    ahead = np.cross(Rl[:, 1], fl)
    ahead = ahead if ahead @ (fl + fr) > 0 else -ahead
    cut = cl + 4.0 * fl
    s = [(*(0.5 * (cl + cr)), 1.2), (*(cl - 3.0 * fl), 0.8), (cut[0], cut[1], 0.2, 0.7), (*(cl + 5.0 * (0.8 * fl + 0.6 * ahead) + 1.0 * up), 0.9),
         (*(cl + 9.0 * (0.8 * fl + 0.6 * ahead) + 2.6 * up), 2.0), (*(cr - 3.0 * fr), 0.8), (*(cr + 4.0 * fr + 1.5 * up), 0.6),
         (*(cl + 15.0 * (0.9 * fl - 0.3 * ahead) + 3.0 * up), 0.5)]
    return np.asarray(s, dtype=np.float32)
