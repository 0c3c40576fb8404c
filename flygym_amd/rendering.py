"""Batch camera renderer: ``HIPSimulation.set_renderer(cam, worlds=[...], use_gpu_batch_rendering=True)``.

The reference's GPU class renders selected worlds with MJWarp's batch ray-caster (``WarpGPUBatchRenderer``,
``warp/rendering.py:279-341``, surface of ``_BaseWarpRenderer`` / ``Renderer``).  Here the ray-caster is
``csrc/nmf_camera.hip``; camera model, scene and shading are build-defined (specification
``tests/camera_spec.py``):

* pinhole cameras; pixel (row, col) has the camera-frame ray ``(u, -v, -1)`` normalised, ``u = (col + 0.5 - W/2) t``,
  ``v = (row + 0.5 - H/2) t``, ``t = tan(fovy/2) / (H/2)``; x right, y up, looking along -z (the eyes' convention);
* mode ``"fixed"``: ``pos`` and ``rotation`` are world coordinates; ``"track"``: position = position of the fly's root
  segment at the rendered step + ``pos``, orientation constant in the world (this build's reading of MuJoCo's ``track``
  for a camera whose parent is the fly's root; unpinned);
* the scene is :class:`flygym_amd.vision.Scene` plus the whole fly — every segment as the capsule fitted to its mesh, each
  with its own colour — lit by one directional light from straight above:
  ``colour = base * (ambient + diffuse * max(0, n_z))``, rounded to uint8.  No shadows, no transparency, no textures.

A world with several flies (one batch per fly) is drawn whole with ``flies="all"`` or a list of fly names: one launch composes
the drawn flies' batches, the nearest hit wins and, on an exact tie, the earlier object — ground, spheres, then capsules in the
order (fly, capsule).  :func:`merge_flies` turns flies, cameras and colours into what the library takes, without a GPU.

Frames are uint8 ``(n_selected_worlds, n_cameras, H, W, 3)`` torch tensors that stay on the device until fetched.
Files are written with Pillow (animated ``.gif`` / ``.png`` / ``.webp``, or a directory of numbered PNGs); other
containers need ``imageio``, :meth:`show_in_notebook` needs ``mediapy`` — neither is a dependency.
"""

from __future__ import annotations

import ctypes
import os
from collections import namedtuple
from pathlib import Path

import numpy as np

from . import _native
from ._handle import NativeHandle, check_params
from .vision import Scene, body_capsules

__all__ = ["HIPBatchRenderer", "CAMERA_MODES", "camera_pose", "resolve_cameras", "select_flies", "merge_flies", "FlyScene", "grid_shape",
           "write_video"]

CAMERA_MODES = {"fixed": 0, "track": 1}
MAX_CAMERAS, MAX_FLIES = 8, 4          # NMF_CAMERA_MAX, NMF_CAMERA_MAX_FLIES of include/nmf.h
PILLOW_SUFFIXES = (".gif", ".png", ".webp")


class _CameraView(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int32), ("track_seg", ctypes.c_int32), ("fovy_deg", ctypes.c_float),
                ("pos", ctypes.c_float * 3), ("rot", ctypes.c_float * 9)]


class _CameraParams(ctypes.Structure):
    _fields_ = [
        ("height", ctypes.c_int32), ("width", ctypes.c_int32), ("cam", _CameraView * 8),
        ("ambient", ctypes.c_float), ("diffuse", ctypes.c_float), ("checker_size", ctypes.c_float),
        ("sky_rgb", ctypes.c_uint8 * 4), ("ground_rgb", (ctypes.c_uint8 * 4) * 2), ("sphere_rgb", (ctypes.c_uint8 * 4) * 8),
        ("n_spheres", ctypes.c_int32), ("spheres_per_world", ctypes.c_int32),
        ("wall_rgb", ctypes.c_uint8 * 4), ("terrain_relief", ctypes.c_int32),
    ]


class _CameraFly(ctypes.Structure):
    """``nmf_camera_fly`` of include/nmf.h."""

    _fields_ = [("batch", ctypes.c_void_p), ("cap_seg", ctypes.c_void_p), ("cap_geom", ctypes.c_void_p), ("cap_rgb", ctypes.c_void_p),
                ("n_caps", ctypes.c_int32)]


def camera_pose(cam: dict):
    """``(mode, position or offset (3,), rotation matrix (3, 3): columns right / up / back, fovy in degrees)`` of a camera
    given as the dict :meth:`Fly.add_tracking_camera` returns.  Refuses every mode but ``"fixed"`` and ``"track"``."""
    from .utils.math import Rotation3D

    mode = cam.get("mode", "fixed")
    if mode not in CAMERA_MODES:
        raise ValueError(f"camera '{cam.get('name')}': mode '{mode}' is not supported; the batch renderer has 'fixed' and 'track'")
    rot = cam.get("rotation")
    if rot is None:
        mat = np.eye(3)
    elif isinstance(rot, Rotation3D):
        mat = rot.as_matrix()
    else:
        mat = np.asarray(rot, dtype=np.float64).reshape(3, 3)
    pos = np.asarray(cam.get("pos", (0.0, 0.0, 0.0)), dtype=np.float64).reshape(3)
    fovy = float(cam.get("fovy", 45.0))
    if not 0.0 < fovy < 180.0:
        raise ValueError(f"camera '{cam.get('name')}': fovy must lie in (0, 180) degrees, got {fovy}")
    return mode, pos, mat, fovy


def resolve_cameras(world, cameras) -> list:
    """``[(fly, camera dict), ...]`` for cameras given as dicts or by name (``"trackcam"`` or ``"<fly name>/trackcam"``),
    one or a list."""
    if not isinstance(cameras, (list, tuple)):
        cameras = [cameras]
    if len(cameras) == 0:
        raise ValueError("At least one valid camera must be specified.")
    flies = world.fly_lookup
    out = []
    for cam in cameras:
        if isinstance(cam, dict):
            owner = next((f for f in flies.values() if any(c is cam for c in f.cameraname_to_camera.values())), None)
            if owner is None:
                owner = next(iter(flies.values()))
            out.append((owner, cam))
            continue
        if not isinstance(cam, str):
            raise ValueError(f"a camera is the dict add_tracking_camera returns or a camera name, got {type(cam).__name__}")
        fly_name, _, cam_name = cam.rpartition("/")
        hits = [(f, f.cameraname_to_camera[cam_name]) for n, f in flies.items()
                if (not fly_name or n == fly_name) and cam_name in f.cameraname_to_camera]
        if len(hits) != 1:
            known = [f"{n}/{c}" for n, f in flies.items() for c in f.cameraname_to_camera]
            raise ValueError(f"camera '{cam}' {'is ambiguous' if hits else 'not found'}; cameras of this world: {known}")
        out.append(hits[0])
    return out


def select_flies(world, flies) -> list:
    """The names of the flies to draw, in ``world.fly_lookup`` order, for ``flies`` = ``"all"``, a fly name or a list of fly
    names.  Unknown, repeated or no names: ``ValueError``, as is more than the renderer's limit of flies."""
    known = list(world.fly_lookup)
    if isinstance(flies, str):
        flies = known if flies == "all" else [flies]
    flies = list(flies)
    if len(flies) == 0:
        raise ValueError("At least one fly must be drawn.")
    for name in flies:
        if name not in known:
            raise ValueError(f"fly '{name}' not found; flies of this world: {known}")
    if len(set(flies)) != len(flies):
        raise ValueError(f"a fly is repeated in {flies}")
    if len(flies) > MAX_FLIES:
        raise ValueError(f"the batch renderer draws at most {MAX_FLIES} flies of a world (NMF_CAMERA_MAX_FLIES), got {len(flies)}")
    return [name for name in known if name in flies]


FlyScene = namedtuple("FlyScene", "fly_names cam_fly track_seg capsule_seg capsule_geom capsule_rgb")
FlyScene.__doc__ = """What :func:`merge_flies` makes of flies, cameras and colours: ``fly_names`` (the drawn flies in the world's
order), per camera ``cam_fly`` (index into ``fly_names`` of the fly it belongs to; 0 for a fixed camera of a fly that is not
drawn) and ``track_seg`` (the tracked segment in that fly's segment order; 0 for fixed cameras), and per drawn fly, in dicts
by fly name, ``capsule_seg`` (K_f,) int32, ``capsule_geom`` (K_f, 7) float32 and ``capsule_rgb`` (K_f, 3) uint8."""


def merge_flies(world, resolved, flies, scene: Scene | None = None, capsule_rgb=None) -> FlyScene:
    """Flies, cameras and colours of one renderer -> the per-fly arrays and per-camera indices the library takes.  Needs no GPU.

    ``resolved``: what :func:`resolve_cameras` returns; ``flies``: see :func:`select_flies`; ``capsule_rgb``: None, or a dict
    fly name -> ``(K_f, 3)`` colours in [0, 1] (flies that are missing get ``scene.body_rgb``).  A ``track`` camera follows its
    own fly, which must be among the drawn ones.  ``ValueError`` for everything that does not fit."""
    scene = scene or Scene()
    names = select_flies(world, flies)
    if len(resolved) > MAX_CAMERAS:
        raise ValueError(f"at most {MAX_CAMERAS} cameras per renderer")
    cam_fly, track_seg = [], []
    for fly, cam in resolved:
        mode = camera_pose(cam)[0]           # (refuses unsupported modes)
        if mode == "track" and fly.name not in names:
            raise ValueError(f"camera '{fly.name}/{cam['name']}' tracks fly '{fly.name}', which is not among the drawn flies {names}")
        cam_fly.append(names.index(fly.name) if fly.name in names else 0)
        segs = [s.name for s in fly.get_bodysegs_order()]
        track_seg.append(segs.index(cam.get("target", fly.root_segment.name)) if mode == "track" else 0)
    if capsule_rgb is None:
        capsule_rgb = {}
    if not isinstance(capsule_rgb, dict):
        raise ValueError("with several flies capsule_rgb is a dict: fly name -> (K, 3) colours")
    for name in capsule_rgb:
        if name not in names:
            raise ValueError(f"capsule_rgb names fly '{name}', which is not among the drawn flies {names}")
    seg, geom, rgb = {}, {}, {}
    for name in names:
        seg[name], geom[name] = (body_capsules(world.fly_lookup[name], hidden=()) if scene.own_body
                                 else (np.zeros(0, np.int32), np.zeros((0, 7), np.float32)))
        k = len(seg[name])
        if capsule_rgb.get(name) is None:
            c = np.tile(np.asarray(scene.body_rgb, dtype=np.uint8), (k, 1))
        else:
            c = np.floor(np.asarray(capsule_rgb[name], dtype=np.float64).reshape(-1, 3) * 255.0 + 0.5).astype(np.uint8)
            if len(c) != k:
                raise ValueError(f"capsule_rgb needs one colour per capsule: ({k}, 3)" + (f" for fly '{name}'" if len(names) > 1 else ""))
        rgb[name] = np.ascontiguousarray(c.reshape(k, 3))
    return FlyScene(names, cam_fly, track_seg, seg, geom, rgb)


def grid_shape(n_worlds: int) -> tuple:
    """(rows, columns) of the near-square grid several worlds are shown in (reference ``warp/rendering.py:219-221``)."""
    n_rows = int(np.ceil(np.sqrt(n_worlds)))
    return n_rows, int(np.ceil(n_worlds / n_rows))


def write_video(path, frames, fps: float, **kwargs) -> Path:
    """Write ``frames`` (a list of (H, W, 3) uint8 arrays) at ``fps``: an animated ``.gif``, ``.png`` (APNG) or ``.webp``
    through Pillow, a directory of numbered PNGs when ``path`` has no suffix; any other suffix through ``imageio`` if it is
    installed, else an ``ImportError`` that names the formats that work."""
    from PIL import Image

    path = Path(path)
    if len(frames) == 0:
        raise RuntimeError("No frames have been recorded yet.")
    suffix = path.suffix.lower()
    if suffix == "":
        path.mkdir(parents=True, exist_ok=True)
        for i, f in enumerate(frames):
            Image.fromarray(np.ascontiguousarray(f)).save(path / f"frame_{i:06d}.png")
        return path
    path.parent.mkdir(parents=True, exist_ok=True)
    if suffix in PILLOW_SUFFIXES:
        images = [Image.fromarray(np.ascontiguousarray(f)) for f in frames]
        extra = {"lossless": True} if suffix == ".webp" else {}
        if suffix == ".gif":
            extra["disposal"] = 1
        images[0].save(path, save_all=True, append_images=images[1:], duration=1000.0 / float(fps), loop=0, **extra)
        return path
    try:
        import imageio
    except ImportError as e:
        raise ImportError(f"writing '{suffix}' needs the imageio package, which is not installed; without it save_video writes "
                          f"{', '.join(PILLOW_SUFFIXES)} (animated, through Pillow) or, for a path without a suffix, a directory of "
                          "numbered PNG frames") from e
    imageio.mimwrite(path, [np.asarray(f) for f in frames], fps=fps, **kwargs)
    return path


class _FrameBuffer:
    """The part of the renderer that needs no GPU: the recorded frames of the selected worlds and cameras, fetching them to
    the host, grids of several worlds, files."""

    def __init__(self, world_ids, camera_names, camera_res=(240, 320), output_fps: float = 25, buffer_frames: bool = True):
        self.world_ids = [int(w) for w in world_ids]
        self.enabled_cam_names = list(camera_names)
        self.camera_res = (int(camera_res[0]), int(camera_res[1]))
        self.output_fps = output_fps
        self.buffer_frames = bool(buffer_frames)
        self._frames = [] if buffer_frames else None

    @property
    def frames(self):
        """The recorded frames: a list of uint8 ``(n_selected_worlds, n_cameras, H, W, 3)`` tensors on the device."""
        return self._frames

    def _camera_index(self, camera) -> int:
        if camera is None:
            if len(self.enabled_cam_names) != 1:
                raise ValueError(f"several cameras were rendered, name one of {self.enabled_cam_names}")
            return 0
        if isinstance(camera, (int, np.integer)):
            if not 0 <= int(camera) < len(self.enabled_cam_names):
                raise ValueError(f"Camera ID '{camera}' not found.")
            return int(camera)
        name = camera.get("name") if isinstance(camera, dict) else str(camera)
        for i, n in enumerate(self.enabled_cam_names):
            if n == name or n.rpartition("/")[2] == name:
                return i
        raise ValueError(f"Camera '{name}' was not among the rendered cameras: {self.enabled_cam_names}")

    def _fetch_frames_to_cpu_oneworld(self, world_id: int, cam_id: int = 0, scale: float | None = None) -> list:
        if not self.buffer_frames:
            raise RuntimeError("Frame buffering was disabled for this renderer, so recorded frames are not available for saving "
                               "or display.")
        if len(self._frames) == 0:
            raise RuntimeError("No frames have been recorded yet.")
        if world_id not in self.world_ids:
            raise ValueError(f"world_id {world_id} was not among the rendered worlds: {self.world_ids}")
        wi, ci = self.world_ids.index(world_id), self._camera_index(cam_id)
        frames = []
        for buf in self._frames:
            f = buf[wi, ci]
            frames.append(f.cpu().numpy() if hasattr(f, "cpu") else np.asarray(f))
        if scale is not None:
            from PIL import Image

            res = tuple(int(x * scale) for x in self.camera_res)
            frames = [np.array(Image.fromarray(f).resize(res[::-1], resample=Image.Resampling.LANCZOS)) for f in frames]
        return frames

    def _fetch_frames_to_cpu_multipleworlds(self, world_ids, cam_id: int = 0, scale: float | None = None) -> list:
        """The worlds side by side in the reference's near-square grid (``warp/rendering.py:215-262``), each labelled with its
        world id (Pillow's default font)."""
        from PIL import Image, ImageDraw, ImageFont

        n_rows, n_cols = grid_shape(len(world_ids))
        if scale is None:
            scale = 1 / n_cols
        res = tuple(int(x * scale) for x in self.camera_res)
        per_world = [self._fetch_frames_to_cpu_oneworld(w, cam_id, scale) for w in world_ids]
        n_frames = len(per_world[0])
        merged = [np.zeros((res[0] * n_rows, res[1] * n_cols, 3), dtype=np.uint8) for _ in range(n_frames)]
        font = ImageFont.load_default()
        for i, (wid, world_frames) in enumerate(zip(world_ids, per_world)):
            row, col = divmod(i, n_cols)
            for j, frame in enumerate(world_frames):
                img = Image.fromarray(frame)
                ImageDraw.Draw(img).text((0.03 * res[1], 0.02 * res[0]), f"World {wid}", font=font, fill=(255, 255, 255))
                merged[j][row * res[0]:(row + 1) * res[0], col * res[1]:(col + 1) * res[1]] = np.array(img)
        return merged

    def _fetch(self, world_id, cam_id, scale):
        if isinstance(world_id, (int, np.integer)):
            return self._fetch_frames_to_cpu_oneworld(int(world_id), cam_id, scale)
        return self._fetch_frames_to_cpu_multipleworlds(list(world_id), cam_id, scale)

    def save_video(self, world_id, output_path, scale: float | None = None, **kwargs) -> None:
        """Save the recorded frames of one world (or a list of worlds, as a grid).  ``output_path``: a path — with several
        cameras a directory that gets one ``<camera>.gif`` each — or a dict camera -> path.  Formats: :func:`write_video`."""
        if isinstance(output_path, dict):
            paths = {self._camera_index(k): Path(v) for k, v in output_path.items()}
        elif len(self.enabled_cam_names) == 1:
            paths = {0: Path(output_path)}
        else:
            paths = {i: Path(output_path) / (n.replace("/", "_") + ".gif") for i, n in enumerate(self.enabled_cam_names)}
        for ci, path in paths.items():
            write_video(path, self._fetch(world_id, ci, scale), self.output_fps, **kwargs)

    def show_in_notebook(self, world_id, camera=None, scale: float | None = None, **kwargs):
        try:
            import mediapy
        except ImportError as e:
            raise ImportError("show_in_notebook needs the mediapy package, which is not installed; save_video writes "
                              f"{', '.join(PILLOW_SUFFIXES)} files that a notebook can display") from e
        cams = range(len(self.enabled_cam_names)) if camera is None else [self._camera_index(camera)]
        for ci in cams:
            mediapy.show_video(self._fetch(world_id, ci, scale), fps=self.output_fps,
                               title=f"world {world_id}, camera {self.enabled_cam_names[ci]}", **kwargs)


class _Pacer:
    """The reference's pacing rule (``warp/rendering.py:96-106``): a frame is due on the first call and then whenever
    ``time >= last + playback_speed / output_fps``.  Time is counted in whole steps of the simulation (``step * timestep``
    compared a billionth of the interval early), so that a frame that is due exactly on a step is not lost to the rounding
    of a sum of floats."""

    def __init__(self, playback_speed: float, output_fps: float):
        if not playback_speed > 0 or not output_fps > 0:
            raise ValueError("playback_speed and output_fps must be positive")
        self.secs_between_renders = float(playback_speed) / float(output_fps)
        self.last_render_time_sec = -np.inf

    def due(self, time_sec: float) -> bool:
        if time_sec >= self.last_render_time_sec + self.secs_between_renders * (1.0 - 1e-9):
            self.last_render_time_sec = time_sec
            return True
        return False

    def reset(self) -> None:
        self.last_render_time_sec = -np.inf


class HIPBatchRenderer(NativeHandle, _FrameBuffer):
    """Renders selected worlds of a :class:`~flygym_amd.HIPSimulation` through one or several cameras, from the poses of the last
    step (``csrc/nmf_camera.hip``: one kernel launch per frame, on the stream the batch is stepped on).

    Args:
        sim: the batch (one fly per world).
        cameras: the dict ``Fly.add_tracking_camera`` returns, a camera name (``"trackcam"`` / ``"<fly name>/trackcam"``), or
            a list of them (at most 8).  A camera dict has ``name``, ``mode`` (``"track"`` / ``"fixed"``), ``pos``,
            ``rotation`` (:class:`Rotation3D`), ``fovy``.
        worlds: indices of the worlds to render, distinct (default: all).
        camera_res: ``(height, width)``.
        playback_speed, output_fps: a frame is due every ``playback_speed / output_fps`` seconds of simulated time.
        buffer_frames: keep the rendered frames (on the device) for :meth:`save_video`.
        scene: a :class:`flygym_amd.vision.Scene` (default: the eyes' default scene).
        ambient, diffuse: the light terms.
        capsule_rgb: ``(K, 3)`` colours in [0, 1], one per segment of the fly (default: ``scene.body_rgb`` for all).
        flies: for a simulation of a world with several flies (:class:`~flygym_amd.simulation.MultiFlyHIPSimulation`, one batch
            per fly): ``"all"`` or a list of fly names — the flies to draw, always in ``world.fly_lookup`` order, at most 4.

    With ``flies`` the image is composed from all drawn flies' batches in one launch (the nearest hit wins; on an exact tie the
    earlier fly).  Cameras may then belong to different flies: a ``track`` camera follows its own fly, which must
    be among the drawn ones.  ``capsule_rgb`` is a dict fly name -> ``(K_f, 3)`` (flies that are missing get
    ``scene.body_rgb``), and the attributes ``capsule_seg``, ``capsule_geom`` and ``capsule_rgb`` are dicts by fly name.  All
    batches of such a simulation step together; pacing (:meth:`render_as_needed`) reads the step counter of the FIRST drawn
    fly's batch.
    """

    _destroy_entry, _noun, _handle_attr = "nmf_camera_plan_destroy", "renderer", "_plan_h"

    def __init__(self, sim, cameras, *, worlds=None, camera_res=(240, 320), playback_speed: float = 0.2, output_fps: float = 25,
                 buffer_frames: bool = True, scene: Scene | None = None, ambient: float = 0.4, diffuse: float = 0.6,
                 capsule_rgb=None, flies=None):
        several = hasattr(sim, "for_fly")
        if several and flies is None:
            raise NotImplementedError("worlds with several flies are drawn on request: pass flies='all' or flies=[fly names] to "
                                      "compose the image from those flies' batches (one batch per fly)")
        if not several and flies is not None:
            raise ValueError("flies= is for a simulation of a world with several flies; this batch steps one fly")
        resolved = resolve_cameras(sim.world, cameras)
        if len(resolved) > MAX_CAMERAS:
            raise ValueError(f"at most {MAX_CAMERAS} cameras per renderer")
        n_worlds = int(sim.n_worlds)
        worlds = list(range(n_worlds)) if worlds is None else [int(w) for w in worlds]
        if len(worlds) == 0:
            raise ValueError("At least one valid world must be specified.")
        for w in worlds:
            if not 0 <= w < n_worlds:
                raise ValueError(f"world id {w} is outside [0, {n_worlds})")
        if len(set(worlds)) != len(worlds):
            raise ValueError(f"a world id is repeated in {worlds}")
        h, w_ = int(camera_res[0]), int(camera_res[1])
        if h < 1 or w_ < 1:
            raise ValueError(f"camera_res must be (height, width) with both at least 1, got {camera_res}")
        sc = scene or Scene()
        if several:
            merged = merge_flies(sim.world, resolved, flies, sc, capsule_rgb)
            batches = [sim.for_fly(name) for name in merged.fly_names]
        else:
            fly = resolved[0][0]
            if any(f is not fly for f, _ in resolved):
                raise NotImplementedError("all cameras of a renderer belong to one fly")
            merged = merge_flies(sim.world, resolved, [fly.name], sc, None if capsule_rgb is None else {fly.name: capsule_rgb})
            batches = [sim]
        poses = [camera_pose(cam) for _, cam in resolved]
        super().__init__(worlds, [f"{f.name}/{cam['name']}" for f, cam in resolved], (h, w_), output_fps, buffer_frames)
        self.sim, self.scene = sim, sc
        self.playback_speed, self.ambient, self.diffuse = float(playback_speed), float(ambient), float(diffuse)
        self._pacer = _Pacer(playback_speed, output_fps)
        self._paced_by = batches[0]
        self.cameras = [cam for _, cam in resolved]
        self.fly_names = merged.fly_names if several else None

        p = _CameraParams()
        p.height, p.width = h, w_
        for i, (mode, pos, mat, fovy) in enumerate(poses):
            v = p.cam[i]
            v.mode, v.fovy_deg, v.track_seg = CAMERA_MODES[mode], fovy, merged.track_seg[i]
            for k in range(3):
                v.pos[k] = pos[k]
            for k in range(9):
                v.rot[k] = mat.reshape(9)[k]
        p.ambient, p.diffuse = self.ambient, self.diffuse
        sc.fill(p)
        if several:
            self.capsule_seg, self.capsule_geom, self.capsule_rgb = merged.capsule_seg, merged.capsule_geom, merged.capsule_rgb
        else:
            self.capsule_seg, self.capsule_geom, self.capsule_rgb = (d[merged.fly_names[0]] for d in merged[3:])
        check_params(_CameraParams, "nmf_camera_params_size", "rendering.py")
        self._params = p
        t = sim._torch
        self._spheres = t.as_tensor(sc.spheres, device=sim.device) if len(sc.spheres) else None
        ids = np.asarray(worlds, dtype=np.int32)
        records = (_CameraFly * len(batches))()
        for rec, name, batch in zip(records, merged.fly_names, batches):
            k = len(merged.capsule_seg[name])
            rec.batch, rec.n_caps = batch._batch_h, k
            if k:
                rec.cap_seg, rec.cap_geom, rec.cap_rgb = (merged[i][name].ctypes.data for i in (3, 4, 5))
        if several:
            cam_fly = np.asarray(merged.cam_fly, dtype=np.int32)
            self._create("nmf_camera_plan_create_flies", records, len(batches), ctypes.byref(p), cam_fly.ctypes.data, len(resolved),
                         ids.ctypes.data, len(ids))
        else:
            one = records[0]
            self._create("nmf_camera_plan_create", one.batch, ctypes.byref(p), len(resolved), ids.ctypes.data, len(ids),
                         one.cap_seg, one.cap_geom, one.cap_rgb, one.n_caps)
        self._shape = (len(worlds), len(resolved), h, w_, 3)

    @staticmethod
    def _creation_error(msg: str) -> Exception:
        return ValueError(msg) if "world id" in msg else _native.NativeError(msg)

    def reset(self) -> None:
        self._pacer.reset()
        if self.buffer_frames:
            self._frames = []

    # ---- rendering
    def set_spheres(self, spheres) -> None:
        """Move the spheres: ``(n_spheres, 4)`` (x, y, z, radius), shared by all worlds; the count must match the scene's."""
        t = self.sim._torch
        s = t.as_tensor(spheres, dtype=t.float32, device=self.sim.device).contiguous()
        if tuple(s.shape) != (len(self.scene.spheres), 4):
            raise ValueError(f"expected spheres of shape ({len(self.scene.spheres)}, 4), got {tuple(s.shape)}")
        self._spheres = s

    def render_into(self, out):
        """Render into a caller-owned contiguous uint8 ``(n_selected_worlds, n_cameras, H, W, 3)`` tensor: no allocation, one
        kernel launch on the current stream — what a captured ``step(n)`` + render replays."""
        plan = self._handle()
        t = self.sim._torch
        if tuple(out.shape) != self._shape or out.dtype != t.uint8 or out.device != self.sim.device or not out.is_contiguous():
            raise ValueError(f"render_into needs a contiguous uint8 {self._shape} tensor on {self.sim.device}")
        spheres = self._spheres.data_ptr() if self._spheres is not None else None
        lib = _native.lib()
        if self.fly_names is None:
            _native.check(lib.nmf_camera_render(self.sim._batch_h, plan, spheres, out.data_ptr(), self.sim._stream()))
        else:
            _native.check(lib.nmf_camera_render_flies(plan, spheres, out.data_ptr(), self.sim._stream()))
        return out

    def render(self):
        """Render now, whatever the pacing says; the frame (a device tensor) is recorded if frames are buffered."""
        t = self.sim._torch
        out = self.render_into(t.empty(self._shape, dtype=t.uint8, device=self.sim.device))
        if self.buffer_frames:
            self._frames.append(out)
        return out

    def render_as_needed(self, sim=None) -> bool:
        """Render if a frame is due (first call; then every ``playback_speed / output_fps`` seconds of simulated time, counted
        from the batch's step counter: no host synchronisation).  With several flies the counter is that of the first drawn
        fly's batch: the batches of such a simulation step together."""
        sim = self._paced_by if sim is None or sim is self.sim else sim
        time_sec = int(_native.lib().nmf_step_count(sim._batch_h)) * sim.timestep
        if not self._pacer.due(time_sec):
            return False
        self.render()
        return True
