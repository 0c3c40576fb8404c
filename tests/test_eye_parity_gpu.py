"""The eye renderer (flygym_amd/csrc/nmf_eyes.hip) against its specification in float64, material by material.

The scene is drawn with colours that name the material (tests/eye_parity.py::PALETTE), so a frame decodes to the kernel's material
per pixel; the float64 flavour of oracle/sensors_oracle.py::render_eye_frames draws the poses read back from the device.  Per frame:

(a) no INTERIOR pixel differs — a pixel whose 3 x 3 neighbourhood has one material in the float64 image.  A float32 ray is 1e-4 of a
    pixel pitch from the float64 one, so a correct kernel differs only where a material boundary passes that close to a pixel centre,
    and such a pixel has a differing neighbour; a wrong cull, a dropped capsule piece or a wrong horizon test differs inside a
    silhouette.  The bar is zero.
(b) interior pixels are at least 0.8 of a 512 x 450 frame and 0.5 of a small one (asserted on the float64 image alone).
(c) all differing pixels of a frame: at most four times the largest share by which the specification in float32 differs from itself
    in float64 (the margin of tests/test_camera_gpu.py: the kernel's float32 is not the specification's — rsq, polynomials, fused
    multiply-adds), never less than 2 pixels.  Full-size frames are held to the largest share among the full-size frames, small
    frames (where one pixel is 1.3e-4 to 3.3e-4 of a frame) to the largest among all frames.
    test_edge_pixels_stay_within_the_bar writes the figures to profiles/eye_parity.txt.
(d) the fused readings equal the resample of the kernel's own frames bit for bit, and an ommatidium's reading is within (its pixels
    that differ) / (its pixels) of the resample of the float64 frame — exact, the palette's bytes staying below 251.
The sampled mode's readings equal ``retina_sampled`` of the pixel-exact frames bit for bit in every case.

Poses are written into ``seg_xpos`` / ``seg_xquat`` (the only fields the kernel reads): a fly after one step, turned about its thorax
and moved, or as it stands after 250 steps.  The float64 frames cost the CPU 1 to 2 s each; the GPU work is milliseconds.

Measured on an MI355X (profiles/eye_parity.txt), 16 full-size and 216 small frames: interior pixels that differ 0; interior share
0.82 to 0.99 (full size) and 0.52 to 0.89 (small); the specification in float32 differs from float64 in 0 to 25 pixels of a full-size
frame (at most 1.09e-4: bar 4.34e-4), the kernel in 0 to 30 (at most 1.30e-4); on small frames both differ in at most 2 pixels
(bar 2.6e-3 of a frame).  The whole module takes 35 s, the slowest test 4.5 s.

What it found: from 1000 mm on a float32 ray parameter no longer moves when the relief walk adds its 1e-4 mm probe step, so a ray
that met the relief that far away stood still for all 64 cells and took the flat answer — in the kernel and in the float32
specification alike, which is why no earlier test saw it.  From 12 mm up that is a band of rows at the horizon: 552 pixels of a
frame, 51 of them interior.  The probe step is now relative beyond 210 mm (nmf_scene.h kTerrainEpsRel, sensors_oracle.TERRAIN_EPS_REL)."""
import functools
from pathlib import Path

import numpy as np
import pytest

import eye_parity as ep
import sensors_oracle as so

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
WORLDS = {"flat": ("FlatGroundWorld", {}), "gapped": ("GappedTerrainWorld", {}), "blocks": ("BlocksTerrainWorld", {}),
          "mixed": ("MixedTerrainWorld", {}),
          # seen from 12 mm the default relief and 4 mm checker squares leave 0.73 of a frame interior: three times the feature size
          # (and 40 mm squares, HIGH_CHECKER) for the case that looks down from there
          "mixed-wide": ("MixedTerrainWorld", dict(block_size=3.9, gap_width=0.9, stripe_length=12.0)),
          # a small retina at 250 or 300 degrees has a pixel pitch of 5 to 6 degrees: on the default blocks (1.3 mm) and checker less than
          # half of a 64 x 48 frame is interior (0.43 to 0.55), on 6 mm blocks and 16 mm squares (SMALL_CHECKER) 0.51 to 0.57
          "blocks-wide": ("BlocksTerrainWorld", dict(block_size=6.0))}
HIGH_CHECKER, SMALL_CHECKER = 40.0, 16.0
TWO_SPHERES = np.array([(6.0, 4.0, 1.5, 1.0), (5.0, -6.0, 0.8, 0.8)], dtype=np.float32)
SMALL, LENS = ep.SMALL_RETINAS, ep.LENS_PATHS


@functools.lru_cache(maxsize=None)
def _batch(key, n_worlds):
    """(sim, fly, segment names, pose after one step, pose after 250 steps) of world 0 — adhesion on; float64 (69, 3) / (69, 4)."""
    import torch
    import flygym_amd.compose as C
    from flygym_amd import HIPSimulation, make_model
    from flygym_amd.utils.math import Rotation3D

    cls, params = WORLDS[key]
    fly, world, _ = make_model()
    if cls != "FlatGroundWorld":
        world = getattr(C, cls)(**params)
        world.add_fly(fly, (0.4, 0.1, 0.8), Rotation3D("quat", (1, 0, 0, 0)))
    sim = HIPSimulation(world, n_worlds=n_worlds, device=0)
    sim.set_leg_adhesion_states(fly.name, np.ones((n_worlds, 6), dtype=np.float32))
    poses = []
    for steps in (1, 249):
        sim.step(steps)
        torch.cuda.synchronize()
        poses.append((sim.field("seg_xpos").cpu().numpy().reshape(n_worlds, 69, 3)[0].astype(np.float64),
                      sim.field("seg_xquat").cpu().numpy().reshape(n_worlds, 69, 4)[0].astype(np.float64)))
    return sim, fly, [s.name for s in fly.get_bodysegs_order()], poses[0], poses[1]


def _write_poses(sim, poses):
    """Write one (xpos, xquat) per world; returns what the device then holds, float64 (n, 69, 3) / (n, 69, 4)."""
    import torch

    n = len(poses)
    for name, k, arr in (("seg_xpos", 3, [p[0] for p in poses]), ("seg_xquat", 4, [p[1] for p in poses])):
        f = sim.field(name)
        f.copy_(torch.as_tensor(np.asarray(arr, dtype=np.float32), device=sim.device).reshape(f.shape))
    torch.cuda.synchronize()
    back = [sim.field(name).cpu().numpy().reshape(n, 69, k).astype(np.float64) for name, k in (("seg_xpos", 3), ("seg_xquat", 4))]
    assert np.array_equal(back[0], np.asarray([p[0] for p in poses], dtype=np.float32))      # the fields are writable views
    return back


def _cameras(fly_names, xpos, xquat):
    from flygym_amd.sensors import EYE_CAMERAS
    from flygym_amd.vision import _euler_xyz_extrinsic_quat

    return [ep.eye_camera(xpos, xquat, fly_names.index(seg), pos, _euler_xyz_extrinsic_quat(euler)) for seg, (pos, euler) in EYE_CAMERAS.items()]


def _scene(spheres, own_body, checker_size=4.0):
    from flygym_amd.vision import Scene

    u = lambda c: tuple(v / 255.0 for v in c)
    return Scene(checker_size=checker_size, sky_rgb=u(ep.PALETTE["sky"]), ground_rgb=tuple(u(c) for c in ep.PALETTE["ground"]),
                 wall_rgb=u(ep.PALETTE["wall"]), body_rgb=u(ep.PALETTE["body"]), spheres=spheres,
                 sphere_rgb=[u(c) for c in ep.PALETTE["spheres"][:len(spheres)]], own_body=own_body)


def _render(label, key, poses, spheres=None, retina=None, fov=157.0, own_body=True, checker_size=4.0):
    """Render the poses (one per world) and lay every frame beside the specification.  ``spheres``: None or float32 (n_worlds, k, 4).
    Returns one record per (world, eye): figures only, nothing is asserted here."""
    import torch
    from flygym_amd.vision import EyeRenderer

    sim, fly, names, _, _ = _batch(key, len(poses))
    xpos, xquat = _write_poses(sim, poses)
    n_sph = 0 if spheres is None else spheres.shape[1]
    scene = _scene(spheres[0] if n_sph else (), own_body, checker_size)
    kw = dict(retina=retina, fov_deg=fov)
    eyes = EyeRenderer(sim, fly.name, scene, **kw)
    sampled = EyeRenderer(sim, fly.name, scene, rays_per_ommatidium=16, **kw)
    if n_sph:
        eyes.set_spheres(spheres)
        sampled.set_spheres(spheres)
    frames, omm = eyes.render_frames(with_readings=True)
    ret = eyes.retina
    fused_equal = bool(torch.equal(omm, ret.raw_image_to_hex_pxls(frames)) and torch.equal(omm, eyes.render()))
    frames, omm, omm_sampled = frames.cpu().numpy(), omm.cpu().numpy(), sampled.render().cpu().numpy()
    fused_equal = fused_equal and np.array_equal(omm, so.retina_resample(frames, ret.id_map, ret.pale_mask, ret.inv_norm))
    sampled_equal = np.array_equal(omm_sampled, so.retina_sampled(frames, ret.id_map, ret.pale_mask))
    terrain = None
    if sim.model["terrain_type"][0] != 0:
        tp = sim.model["terrain_params"]
        terrain = (int(sim.model["terrain_type"][0]), tuple(float(v) for v in tp[:4]), float(tp[4]))
    H, W = ret.height, ret.width
    ids = ret.id_map.ravel().astype(np.int64)
    counts = np.bincount(ids, minlength=ret.num_ommatidia + 1)[1:]
    records = []
    for w in range(len(poses)):
        caps = ep.world_capsules(xpos[w], xquat[w], eyes.capsule_seg, eyes.capsule_geom) if own_body else []
        for e, (cam, R) in enumerate(_cameras(names, xpos[w], xquat[w])):
            sph = spheres[w] if n_sph else ()
            frame64, mat64 = ep.spec_view(cam, R, H, W, fov, terrain, sph, caps, np.float64, checker_size)
            _, mat32 = ep.spec_view(cam, R, H, W, fov, terrain, sph, caps, np.float32, checker_size)
            got = ep.decode_materials(frames[w, e], n_sph)
            interior, differ = ep.interior_mask(mat64), got != mat64
            ref = so.retina_resample(frame64, ret.id_map, ret.pale_mask, ret.inv_norm)
            allowed = np.bincount(ids, weights=differ.ravel(), minlength=ret.num_ommatidia + 1)[1:] / counts
            records.append(dict(
                label=f"{label} world {w} eye {e}", n_pix=H * W, full=(H, W) == (512, 450), cam=cam, mat64=mat64, got=got,
                interior_share=float(interior.mean()), spec_differ=int((mat32 != mat64).sum()), differ=int(differ.sum()),
                interior_differ=int((differ & interior).sum()), fused_equal=fused_equal, sampled_equal=bool(sampled_equal),
                reading_excess=float((np.abs(omm[w, e] - ref).max(axis=-1) - allowed).max())))
    return tuple(records)


def _check(records, min_interior):
    """(b), then (a), (d) and the sampled mode, of every frame of a case."""
    for r in records:
        print(f"eye parity {r['label']}: interior share {r['interior_share']:.3f}; of {r['n_pix']} pixels the specification in float32 "
              f"differs from float64 in {r['spec_differ']}, the kernel in {r['differ']} ({r['interior_differ']} interior)")
    for r in records:
        assert r["interior_share"] >= min_interior, r["label"]
    for r in records:
        assert r["interior_differ"] == 0, f"{r['label']}: {r['interior_differ']} interior pixels differ from the float64 specification"
        assert r["fused_equal"], f"{r['label']}: fused readings differ from the resample of the frames"
        assert r["reading_excess"] <= 0.0, f"{r['label']}: a reading is {r['reading_excess']:.2e} beyond its differing pixels"
        assert r["sampled_equal"], f"{r['label']}: the sampled mode differs from retina_sampled of the pixel-exact frames"


def _share(mat, *materials):
    return float(np.isin(mat, materials).mean())


# ---- full retina: 512 x 450, 157 degrees, own body, two spheres; one world per case
@functools.lru_cache(maxsize=None)
def _full_case(name):
    if name.startswith("standing-"):
        key = name.split("-", 1)[1]
        pose = _batch(key, 1)[4]
        return _render(name, key, [pose], TWO_SPHERES[None])
    key, checker = {"upside-down": ("flat", 4.0), "nose-up": ("flat", 4.0), "high": ("mixed-wide", HIGH_CHECKER), "in-gap": ("gapped", 4.0)}[name]
    _, _, names, (xpos, xquat), _ = _batch(key, 1)
    if name == "upside-down":
        pose = ep.move_rigidly(xpos, xquat, (1, 0, 0), 180.0, (None, None, 3.0))
    elif name == "nose-up":
        pose = ep.move_rigidly(xpos, xquat, (0, 1, 0), -90.0, (None, None, 3.0))
    elif name == "high":
        pose = ep.move_rigidly(xpos, xquat, (0, 0, 1), 30.0, (None, None, 12.0))
    else:     # both eyes 0.5 mm below the tops, in the middle of the 0.3 mm gap that spans x = 1.0 .. 1.3
        mid = np.mean([c for c, _ in _cameras(names, xpos, xquat)], axis=0)
        pose = ep.move_rigidly(xpos, xquat, (0, 0, 1), 0.0, tuple(xpos[0] + np.array([1.15, mid[1], -0.5]) - mid))
    return _render(name, key, [pose], TWO_SPHERES[None], checker_size=checker)


FULL_CASES = ("standing-flat", "standing-gapped", "standing-blocks", "standing-mixed", "upside-down", "nose-up", "high", "in-gap")


@pytest.mark.parametrize("name", FULL_CASES)
def test_full_retina_matches_the_float64_specification(name):
    """The fly as it stands after 250 steps on each terrain; rolled upside down 3 mm above flat ground (the eyes' upper halves see the
    ground); pitched nose-up there (the horizon runs down the image: one half has no ground); 12 mm above a mixed terrain, turned 30
    degrees (rays near the horizon run out of the 64-cell walk and keep the flat answer); both eyes inside a gap, below the tops (walls at
    close range)."""
    records = _full_case(name)
    assert len(records) == 2
    _check(records, 0.8)
    mats = [r["mat64"] for r in records]
    for r, m in zip(records, mats):
        assert _share(m, 4) > 0.01, r["label"]                                # the fly's own body is in view
        if name == "standing-flat":
            assert _share(m, 3) == 0.0 and _share(m, 1, 2) > 0.2
        elif name.startswith("standing-"):
            assert _share(m, 3) > 0.002, r["label"]                            # side walls of the relief
        elif name == "upside-down":
            assert _share(m[:256], 1, 2) > 0.6 > 0.2 > _share(m[256:], 1, 2), r["label"]
        elif name == "nose-up":
            halves = sorted((_share(m[:, :225], 1, 2), _share(m[:, 225:], 1, 2)))
            assert halves[0] < 0.02 and halves[1] > 0.2, r["label"]
        elif name == "high":
            assert abs(r["cam"][2] - 12.0) < 0.5 and _share(m, 3) > 0.02 and _share(m, 1, 2) > 0.2, r["label"]
        elif name == "in-gap":
            assert r["cam"][2] < -0.3 and 1.0 < r["cam"][0] < 1.3 and _share(m, 3) > 0.3, r["label"]
    if name in ("standing-flat", "upside-down", "nose-up"):
        assert any(_share(m, 5, 6) > 0.002 for m in mats)                      # a sphere is in view of an eye


# ---- small retinas: rectangular lattices, three sizes, four lenses, flat and blocks terrain, two worlds
@functools.lru_cache(maxsize=None)
def _retina(shape):
    from flygym_amd.sensors import Retina

    rows, cols = SMALL[shape]
    id_map = ep.lattice_id_map(*shape, rows, cols, seed=shape[1])
    return Retina(id_map=id_map, pale_mask=np.random.default_rng(shape[0]).integers(0, 2, rows * cols))


def _small_poses(key):
    """World 0 as the fly stands; world 1 turned (yaw 40, then roll 10 degrees) and moved aside."""
    _, _, _, (xpos, xquat), standing = _batch(key, 2)
    turned = ep.move_rigidly(*ep.move_rigidly(xpos, xquat, (0, 0, 1), 40.0, (None, None, None)), (1, 0, 0), 10.0, (xpos[0, 0] + 0.7, xpos[0, 1] - 0.5, None))
    return [standing, turned]


def _eight(key, poses):
    """Eight spheres per world, placed about that world's cameras (world 1's also 5 % larger)."""
    names = _batch(key, 2)[2]
    out = np.stack([ep.eight_spheres(_cameras(names, *p)) for p in poses])
    out[1, :, 3] *= 1.05
    return out


@functools.lru_cache(maxsize=None)
def _small_case(shape, fov):
    records = []
    for key in ("flat", "blocks-wide"):
        poses = _small_poses(key)
        label = f"{shape[1]}x{shape[0]} fov {fov} {key}"
        kw = dict(retina=_retina(shape), fov=float(fov), checker_size=SMALL_CHECKER)
        records += _render(f"{label} no spheres", key, poses, None, **kw)
        records += _render(f"{label} eight spheres", key, poses, _eight(key, poses), **kw)
        if fov == 157:      # no capsule while spheres are culled
            records += _render(f"{label} eight spheres, no body", key, poses, _eight(key, poses), own_body=False, **kw)
    return tuple(records)


SMALL_CASES = [(shape, fov) for shape in SMALL for fov in (140, 157, 250, 300)]


@pytest.mark.parametrize("shape, fov", SMALL_CASES, ids=[f"{s[1]}x{s[0]}-{f}" for s, f in SMALL_CASES])
def test_small_retina_matches_the_float64_specification(shape, fov):
    """64 x 48 (width a multiple of 16: no chunk wraps; 3072 pixels, a multiple of 1024), 50 x 64 (most chunks wrap), 96 x 80 (7680
    pixels, no multiple of 1024) at 140 / 157 / 250 / 300 degrees (LENS: polynomial path or not, black corners or not), on flat and
    blocks terrain (6 mm blocks, 16 mm checker squares), two worlds, the own body on: no sphere; eight spheres placed per world (one encloses both cameras, one sits
    directly behind each eye, one is cut by the ground, two overlap at different depths); at 157 degrees also eight spheres and no body."""
    records = _small_case(shape, fov)
    assert len(records) == (24 if fov == 157 else 16)
    _check(records, 0.5)
    lens_ok, n_black = LENS[shape][fov]
    for r in records:
        assert int((r["mat64"] == -1).sum()) == n_black and abs(int((r["got"] == -1).sum()) - n_black) <= 2, r["label"]
        if "eight" in r["label"]:
            assert not (r["mat64"] == 5).any(), r["label"]                      # the sphere around the cameras is not seen
    eight = [r for r in records if "eight spheres" in r["label"] and "no body" not in r["label"]]
    seen = set().union(*(set(np.unique(r["mat64"]).tolist()) for r in eight))
    assert {7, 8, 9} <= seen                      # the cut sphere and the overlapping pair are in view


def test_more_than_eight_spheres_are_refused():
    from flygym_amd.vision import EyeRenderer

    nine = np.tile(TWO_SPHERES[0], (9, 1))
    with pytest.raises(ValueError):
        _scene(nine, True)
    sim, fly, _, _, standing = _batch("flat", 2)
    _write_poses(sim, [standing, standing])
    eyes = EyeRenderer(sim, fly.name, _scene(nine[:8], True), retina=_retina((48, 64)))
    with pytest.raises(ValueError):
        eyes.set_spheres(nine)
    with pytest.raises(ValueError):
        eyes.set_spheres(np.tile(nine[None], (2, 1, 1)))


def test_edge_pixels_stay_within_the_bar():
    """(c) over every frame of this module (cases other tests rendered are reused), and the report profiles/eye_parity.txt."""
    records = [r for name in FULL_CASES for r in _full_case(name)] + [r for shape, fov in SMALL_CASES for r in _small_case(shape, fov)]
    worst_full = max(r["spec_differ"] / r["n_pix"] for r in records if r["full"])
    worst_all = max(r["spec_differ"] / r["n_pix"] for r in records)
    lines = ["eye renderer against its float64 specification (tests/test_eye_parity_gpu.py): pixels whose material differs, per frame",
             "frame | pixels | interior share | float32 specification: pixels, share | kernel: pixels, share, interior pixels | bar (share)"]
    failed = []
    for r in records:
        bar = max(4.0 * (worst_full if r["full"] else worst_all), 2.0 / r["n_pix"])
        lines.append(f"{r['label']} | {r['n_pix']} | {r['interior_share']:.3f} | {r['spec_differ']}, {r['spec_differ'] / r['n_pix']:.2e} | "
                     f"{r['differ']}, {r['differ'] / r['n_pix']:.2e}, {r['interior_differ']} | {bar:.2e}")
        if r["differ"] / r["n_pix"] > bar:
            failed.append(r["label"])
    lines.append(f"largest float32-specification share: full-size frames {worst_full:.2e} (bar {max(4 * worst_full, 2 / 230400):.2e}), "
                 f"all frames {worst_all:.2e} (bar of a small frame {4 * worst_all:.2e}, never below 2 pixels)")
    lines.append(f"largest kernel share: full-size frames {max(r['differ'] / r['n_pix'] for r in records if r['full']):.2e}, "
                 f"small frames {max(r['differ'] / r['n_pix'] for r in records if not r['full']):.2e}; "
                 f"interior pixels that differ: {sum(r['interior_differ'] for r in records)}")
    print("\n".join(lines))
    try:
        (ROOT / "profiles" / "eye_parity.txt").write_text("\n".join(lines) + "\n")
    except OSError:
        pass                                    # (a read-only checkout: the figures are printed above)
    assert not failed, failed
