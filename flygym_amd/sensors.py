"""Vision and olfaction sensors on the GPU.

The reference snapshot keeps only the constants of flygym 1.x's retina and odor sensors
(``src/flygym/assets/model/legacy/flygym1_config.yaml:141-192``): 721 ommatidia per eye, 512 x 450 raw
eye images, eye-camera placement, four odor sensor sites.  The ommatidia id map and pale-type mask files it
names (``:199-200``) are not shipped, and no code exists, so the following is *build-defined*:

* the id map is a flat-top hexagonal lattice of radius 15 (3*15*16 + 1 = 721 cells) whose circum-size makes
  it span the 512-pixel height (it then spans 448 of the 450 columns); a pixel belongs to the cell whose
  centre is nearest, or to none outside the hexagon; ids run row-major over cell centres;
* 30 % of the ommatidia are "pale" (read the blue channel), the rest "yellow" (read green), drawn once with
  ``numpy.random.default_rng(0)``;
* a reading is the mean of the cell's pixels in its channel / 255, stored in channel 0 (yellow) or 1 (pale);
* odor intensity = sum over sources of ``peak / distance**2`` at the four sensor sites (:class:`OdorSensors`), or the reading
  of a time-varying plume grid per world, advected by a noisy wind beside the physics (:class:`OdorPlume`; the reference holds
  no plume code or data: the whole model is stated in include/nmf.h and specified by tests/plume_spec.py);
* path integration (:class:`PathIntegrator`) — heading and position from the legs' stance strides, in the form of flygym 1.x's
  path-integration task — is stated in include/nmf.h and specified by tests/odometry_spec.py;
* motion vision (:class:`MotionDetectors`) — two low-pass filters per ommatidium, a Hassenstein-Reichardt correlator per pair of
  neighbouring ommatidia (:meth:`Retina.motion_pairs`), wide-field flow per eye and an optomotor drive for the ``TurningCPG`` — is
  stated in include/nmf.h and specified by tests/motion_spec.py; the reference holds no vision processing at all;
* a retinotopic visual network (:class:`RetinotopicNetwork`) — cell types as layers of one cell per ommatidium, joined by
  convolution kernels on the hexagonal lattice (:meth:`Retina.hex_neighbours`), a leaky recurrent system whose pooled activity
  steers the ``TurningCPG``; :func:`motion_pathway` is its default network — is stated in include/nmf.h and specified by
  tests/visnet_spec.py.

The arithmetic runs in ``libnmf_hip.so`` (``nmf_retina_resample``, ``nmf_odor_intensity``, ``nmf_plume_*``, ``nmf_odometry_*``,
``nmf_motion_*``, ``nmf_visnet_*``).
"""

from __future__ import annotations

import ctypes
from dataclasses import dataclass, field

import numpy as np

from . import _native
from ._handle import NativeHandle, _field_view, check_params, fly_batch, leg_segments, reset_mask, site_arrays
from .anatomy import LEGS

__all__ = ["Retina", "OdorSensors", "OdorPlume", "PathIntegrator", "MotionDetectors", "RetinotopicNetwork", "VisualNetwork", "FlatNetwork", "motion_pathway",
           "flatten_network", "eye_tables", "RAW_IMG_HEIGHT", "RAW_IMG_WIDTH", "NUM_OMMATIDIA"]

RAW_IMG_HEIGHT = 512     # flygym1_config.yaml:143
RAW_IMG_WIDTH = 450      # :144
NUM_OMMATIDIA = 721      # :145
FOVY_PER_EYE_DEG = 157   # :142
EYE_CAMERAS = {          # :164-173  (parent segment, offset mm, euler orientation)
    "l_eye": ((-0.03, 0.38, 0.0), (1.57, 0.00, -0.47)),
    "r_eye": ((-0.03, -0.38, 0.0), (-1.57, 3.14, 0.47)),
}
MAX_STEERING_SIDE = 2047          # csrc/nmf_taxis.hip: ommatidium centres are int16 sixteenths of a pixel ...
MAX_STEERING_OMMATIDIA = 1024     # ... and at most kMaxOmmatidia of them are summed
MAX_MOTION_PAIRS = 3072           # csrc/nmf_motion.hip: pairs of neighbouring ommatidia an eye's int32 flow sums can hold
MAX_VISNET_TYPES, MAX_VISNET_CELLS, MAX_VISNET_TABLE = 32, 24576, 19      # csrc/nmf_visnet.hip: what one CU's LDS holds ...
MAX_VISNET_EDGES, MAX_VISNET_TAPS, MAX_VISNET_SUBSTEPS = 512, 4096, 8     # ... and the limits of include/nmf.h
ODOR_SENSOR_SITES = [    # :175-192  (parent segment, offset in the segment frame, mm)
    ("c_rostrum", (-0.15, 0.15, -0.15)),     # left maxillary palp
    ("c_rostrum", (-0.15, -0.15, -0.15)),    # right maxillary palp
    ("l_funiculus", (0.02, 0.00, -0.10)),    # left antenna
    ("r_funiculus", (0.02, 0.00, -0.10)),    # right antenna
]


def make_ommatidia_id_map(height: int = RAW_IMG_HEIGHT, width: int = RAW_IMG_WIDTH, radius: int = 15) -> np.ndarray:
    """(height, width) int16 map: 0 = no ommatidium, k = ommatidium k-1."""
    size = height / ((2 * radius + 1) * np.sqrt(3.0))          # hexagon spans the image height
    cells = [(q, r) for q in range(-radius, radius + 1) for r in range(-radius, radius + 1) if abs(q + r) <= radius]
    centres = np.array([(size * 1.5 * q, size * np.sqrt(3.0) * (r + 0.5 * q)) for q, r in cells])   # (x, y)
    order = np.lexsort((centres[:, 0], centres[:, 1]))          # row-major over centres: y, then x
    ident = {cells[i]: k + 1 for k, i in enumerate(order)}
    ys, xs = np.mgrid[0:height, 0:width]
    px = xs + 0.5 - 0.5 * width
    py = ys + 0.5 - 0.5 * height
    qf = (2.0 / 3.0) * px / size
    rf = (-1.0 / 3.0 * px + np.sqrt(3.0) / 3.0 * py) / size
    x, z = qf, rf
    y = -x - z
    rx, ry, rz = np.rint(x), np.rint(y), np.rint(z)
    dx, dy, dz = np.abs(rx - x), np.abs(ry - y), np.abs(rz - z)
    fix_x = (dx > dy) & (dx > dz)
    fix_y = ~fix_x & (dy > dz)
    rx = np.where(fix_x, -ry - rz, rx)
    rz = np.where(~fix_x & ~fix_y, -rx - ry, rz)
    q, r = rx.astype(int), rz.astype(int)
    inside = (np.abs(q) <= radius) & (np.abs(r) <= radius) & (np.abs(q + r) <= radius)
    out = np.zeros((height, width), dtype=np.int16)
    lut = np.zeros((2 * radius + 1, 2 * radius + 1), dtype=np.int16)
    for (cq, cr), k in ident.items():
        lut[cq + radius, cr + radius] = k
    out[inside] = lut[q[inside] + radius, r[inside] + radius]
    return out


class Retina:
    """Compound-eye model: raw eye images -> ommatidia readings, batched on the GPU."""

    def __init__(self, id_map: np.ndarray | None = None, pale_mask: np.ndarray | None = None, pale_fraction: float = 0.3):
        self.id_map = make_ommatidia_id_map() if id_map is None else np.ascontiguousarray(id_map, dtype=np.int16)
        self.height, self.width = self.id_map.shape
        self.num_ommatidia = int(self.id_map.max())
        counts = np.bincount(self.id_map.ravel(), minlength=self.num_ommatidia + 1)[1:]
        if (counts == 0).any():
            raise ValueError("every ommatidium needs at least one pixel")
        self.num_pixels_per_ommatidium = counts
        if pale_mask is None:
            pale_mask = np.random.default_rng(0).random(self.num_ommatidia) < pale_fraction
        self.pale_mask = np.ascontiguousarray(pale_mask, dtype=np.uint8)
        self.inv_norm = (1.0 / (255.0 * counts)).astype(np.float32)
        self._dev = None

    def _device_constants(self, torch, device):
        if self._dev is None or self._dev[0] != device:
            ids = self.id_map.ravel().astype(np.int64)
            typed = ids | (np.where(ids > 0, self.pale_mask[np.maximum(ids, 1) - 1], 0).astype(np.int64) << 15)
            id_dev = torch.as_tensor(typed.astype(np.uint16).view(np.int16), device=device)
            plan = None
            if typed.size % 16 == 0:      # run plan of the id map (streaming kernel); built once per device
                plan = torch.empty(_native.lib().nmf_retina_plan_bytes(typed.size), dtype=torch.uint8, device=device)
                stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
                _native.check(_native.lib().nmf_retina_plan(id_dev.data_ptr(), typed.size, plan.data_ptr(), stream))
            self._dev = (device, id_dev, torch.as_tensor(self.pale_mask, device=device),
                         torch.as_tensor(self.inv_norm, device=device), plan)
        return self._dev[1:]

    def raw_image_to_hex_pxls(self, images):
        """``images``: torch uint8 tensor ``(..., height, width, 3)`` on the GPU ->
        float32 ``(..., num_ommatidia, 2)`` (channel 0 = yellow-type reading, 1 = pale-type reading)."""
        import torch

        if images.dtype != torch.uint8 or images.shape[-3:] != (self.height, self.width, 3):
            raise ValueError(f"expected uint8 images of shape (..., {self.height}, {self.width}, 3), got {tuple(images.shape)}")
        if not images.is_cuda:
            raise _native.NativeError("the retina resample runs on the MI355X: pass a GPU tensor")
        images = images.contiguous()
        lead = tuple(images.shape[:-3])
        n = int(np.prod(lead)) if lead else 1
        id_map, pale, inv_norm, plan = self._device_constants(torch, images.device)
        out = torch.empty(lead + (self.num_ommatidia, 2), dtype=torch.float32, device=images.device)
        stream = ctypes.c_void_p(torch.cuda.current_stream(images.device).cuda_stream)
        _native.check(_native.lib().nmf_retina_resample(
            images.data_ptr(), id_map.data_ptr(), plan.data_ptr() if plan is not None else None, pale.data_ptr(),
            inv_norm.data_ptr(), n,
            self.height * self.width, self.num_ommatidia, out.data_ptr(), stream))
        return out

    def ommatidia_centres(self) -> np.ndarray:
        """float64 ``(num_ommatidia, 2)``: the mean ``(x, y)`` of the pixel centres ``(col + 1/2, row + 1/2)`` of each
        ommatidium's cell in :attr:`id_map`."""
        ids = self.id_map.ravel().astype(np.int64)
        rows, cols = np.divmod(np.arange(ids.size), self.width)
        counts = self.num_pixels_per_ommatidium.astype(np.float64)
        x = np.bincount(ids, weights=cols + 0.5, minlength=self.num_ommatidia + 1)[1:] / counts
        y = np.bincount(ids, weights=rows + 0.5, minlength=self.num_ommatidia + 1)[1:] / counts
        return np.stack([x, y], axis=-1)

    def centre_table(self) -> np.ndarray:
        """int16 ``(num_ommatidia, 2)``: :meth:`ommatidia_centres` in sixteenths of a pixel, ``rint(16 * centre)`` — the table
        the steering kernel sums (``controllers.SensorySteering``).  Refuses a retina that does not fit it."""
        if max(self.height, self.width) > MAX_STEERING_SIDE:
            raise ValueError(f"a retina of {self.height} x {self.width} pixels exceeds {MAX_STEERING_SIDE} a side (int16 sixteenths of a pixel)")
        if self.num_ommatidia > MAX_STEERING_OMMATIDIA:
            raise ValueError(f"a retina of {self.num_ommatidia} ommatidia exceeds the steering kernel's {MAX_STEERING_OMMATIDIA}")
        return np.rint(16.0 * self.ommatidia_centres()).astype(np.int16)

    def motion_pairs(self, reach: float = 1.25):
        """``(pairs (P, 2) int32, weights (P, 2) float32)``: every pair ``a < b`` of ommatidia whose centres
        (:meth:`ommatidia_centres`) are closer than ``reach`` times the median nearest-neighbour distance, in ascending
        ``(a, b)``, and the unit vector from ``a`` to ``b`` in image coordinates (x = column, y = row) — the neighbour list the
        motion detectors correlate over (:class:`MotionDetectors`).  The default retina: 2070 pairs along the lattice's three
        axes.  Refuses a retina with more than 3072 pairs or more than 1024 ommatidia."""
        if self.num_ommatidia > MAX_STEERING_OMMATIDIA:
            raise ValueError(f"a retina of {self.num_ommatidia} ommatidia exceeds the motion kernel's {MAX_STEERING_OMMATIDIA}")
        c = self.ommatidia_centres()
        if c.shape[0] < 2:
            return np.zeros((0, 2), dtype=np.int32), np.zeros((0, 2), dtype=np.float32)
        v = c[None, :, :] - c[:, None, :]                          # v[a, b] = centre b - centre a
        dist = np.hypot(v[..., 0], v[..., 1])
        pitch = np.median(np.where(np.eye(c.shape[0], dtype=bool), np.inf, dist).min(axis=1))
        a, b = np.nonzero(np.triu(dist < float(reach) * pitch, k=1))      # (row-major: ascending a, then b)
        if a.size > MAX_MOTION_PAIRS:
            raise ValueError(f"{a.size} pairs within {reach} pitches exceed the motion kernel's {MAX_MOTION_PAIRS}")
        weights = v[a, b] / dist[a, b, None]
        return np.stack([a, b], axis=-1).astype(np.int32), weights.astype(np.float32)

    def hex_neighbours(self, rings: int = 2):
        """``(neighbours (T, num_ommatidia) int32, offsets (T, 2) float64)``, ``T`` = 1, 7 or 19 for ``rings`` = 0, 1, 2: the
        hexagonal lattice of the retina as a table, the taps a :class:`RetinotopicNetwork` convolves over.  ``offsets[t]`` is a
        lattice vector in image coordinates (x = column, y = row) and ``neighbours[t, i]`` the ommatidium whose centre lies within
        a quarter of a pitch of ``centre_i + offsets[t]``, or -1 where the retina ends.

        Derived from :meth:`ommatidia_centres`: the displacements from the ommatidium nearest the centroid to its six nearest
        neighbours give the pitch (their mean length) and two lattice vectors 60 degrees apart; the taps are their integer
        combinations within 2.05 pitches of zero — tap 0 the cell itself, then the classes at distance 1, sqrt(3) and 2 pitches,
        each in ascending ``atan2(dy, dx)``.  ``rings`` = 1 keeps the first class, 2 all three.  The default retina: 690
        ommatidia have any one distance-1 tap, 660 a distance-sqrt(3) tap and 659 a distance-2 tap; 547 have all 19.

        Refuses (``ValueError``) more than 1024 ommatidia, fewer than 7 when ``rings`` > 0, and a retina that is not a hexagonal
        lattice: the combinations do not fall into classes of six at 1, sqrt(3) and 2 pitches, or a target has an ommatidium
        between 0.25 and 0.75 pitch from it."""
        if rings not in (0, 1, 2):
            raise ValueError(f"rings must be 0, 1 or 2, got {rings!r}")
        n = self.num_ommatidia
        if n > MAX_STEERING_OMMATIDIA:
            raise ValueError(f"a retina of {n} ommatidia exceeds the network kernel's {MAX_STEERING_OMMATIDIA}")
        if rings == 0:
            return np.arange(n, dtype=np.int32)[None, :].copy(), np.zeros((1, 2))
        if n < 7:
            raise ValueError(f"a retina of {n} ommatidia has no hexagonal neighbourhood (rings > 0 needs at least 7)")
        c = self.ommatidia_centres()
        middle = int(np.argmin(np.hypot(*(c - c.mean(axis=0)).T)))
        d = c - c[middle]
        six = d[np.argsort(np.hypot(d[:, 0], d[:, 1]), kind="stable")[1:7]]
        pitch = float(np.hypot(six[:, 0], six[:, 1]).mean())
        angle = np.arctan2(six[:, 1], six[:, 0])
        first = int(np.argmin(angle))
        turn = (angle - angle[first]) % (2.0 * np.pi)
        at = lambda want: six[int(np.argmin(np.abs(turn - want)))]             # the neighbour `want` radians on from the first
        a, b = 0.5 * (at(0.0) - at(np.pi)), 0.5 * (at(np.pi / 3.0) - at(4.0 * np.pi / 3.0))      # (each with its opposite)
        grid = np.array([(m, k) for m in range(-3, 4) for k in range(-3, 4)], dtype=np.float64)
        points = grid[:, :1] * a + grid[:, 1:] * b
        dist = np.hypot(points[:, 0], points[:, 1]) / pitch
        points, dist = points[dist < 2.05], dist[dist < 2.05]
        classes = [points[np.abs(dist - want) < 0.1] for want in (0.0, 1.0, np.sqrt(3.0), 2.0)]
        if [len(k) for k in classes] != [1, 6, 6, 6] or len(points) != 19:
            raise ValueError("the retina is not a hexagonal lattice: the neighbours of its middle ommatidium do not span one")
        offsets = np.concatenate([k[np.argsort(np.arctan2(k[:, 1], k[:, 0]), kind="stable")] for k in classes])
        offsets[0] = 0.0
        offsets = offsets[:7] if rings == 1 else offsets
        neighbours = np.full((len(offsets), n), -1, dtype=np.int32)
        for t, off in enumerate(offsets):
            target = c + off
            gap = np.hypot(target[:, None, 0] - c[None, :, 0], target[:, None, 1] - c[None, :, 1]) / pitch        # [i, j]
            if ((gap >= 0.25) & (gap < 0.75)).any():
                i, j = np.argwhere((gap >= 0.25) & (gap < 0.75))[0]
                raise ValueError(f"the retina is not a hexagonal lattice: ommatidium {j} lies {gap[i, j]:.2f} pitch from tap {t} of ommatidium {i}")
            j = gap.argmin(axis=1)
            hit = gap[np.arange(n), j] < 0.25
            neighbours[t, hit] = j[hit]
        return neighbours, offsets

    def hex_pxls_to_human_readable(self, readings: np.ndarray) -> np.ndarray:
        """Paint ``(num_ommatidia, 2)`` readings back onto the pixel grid (for inspection)."""
        vals = np.concatenate([[0.0], np.asarray(readings).max(axis=-1)])
        return vals[self.id_map]


class OdorSensors:
    """The fly's four odor sensors (two maxillary palps, two antennae) in an odor field of point sources."""

    def __init__(self, sim, fly_name: str, source_positions, peak_intensities):
        import torch

        self.sim = sim = fly_batch(sim, fly_name, resolve=True)
        seg, rel = site_arrays(sim.world.fly_lookup[fly_name], ODOR_SENSOR_SITES)
        self.source_positions = np.asarray(source_positions, dtype=np.float32).reshape(-1, 3)
        self.peak_intensities = np.asarray(peak_intensities, dtype=np.float32).reshape(len(self.source_positions), -1)
        self.n_dims = self.peak_intensities.shape[1]
        dev = sim.device
        self._seg, self._rel = torch.as_tensor(seg, device=dev), torch.as_tensor(rel, device=dev)
        self._pos = torch.as_tensor(self.source_positions, device=dev)
        self._peak = torch.as_tensor(self.peak_intensities, device=dev)

    def get_odor_intensities(self):
        """float32 ``(n_worlds, n_dims, 4)`` from the poses of the last step."""
        import torch

        out = torch.empty((self.sim.n_worlds, self.n_dims, 4), dtype=torch.float32, device=self.sim.device)
        _native.check(_native.lib().nmf_odor_intensity(
            self.sim._batch_h, self._seg.data_ptr(), self._rel.data_ptr(), 4, self._pos.data_ptr(),
            self._peak.data_ptr(), len(self.source_positions), self.n_dims, out.data_ptr(), self.sim._stream()))
        return out


class _PlumeParams(ctypes.Structure):
    """``nmf_plume_params`` of include/nmf.h."""

    _fields_ = [("n_plumes", ctypes.c_int32), ("height", ctypes.c_int32), ("width", ctypes.c_int32), ("first_world", ctypes.c_int32),
                ("cell_size", ctypes.c_float), ("origin_x", ctypes.c_float), ("origin_y", ctypes.c_float), ("tick_s", ctypes.c_float),
                ("diffusivity", ctypes.c_float), ("mean_wind_x", ctypes.c_float), ("mean_wind_y", ctypes.c_float),
                ("wind_tau", ctypes.c_float), ("wind_sigma", ctypes.c_float), ("eddy_gain", ctypes.c_float),
                ("intensity_scale", ctypes.c_float), ("seed", ctypes.c_uint32)]


class OdorPlume(NativeHandle):
    """Time-varying odor plumes on the GPU, one per world, and the fly's four odor sensors in them (``nmf_plume_*``).

    A plume is a float32 concentration grid over the ground plane (cell ``(j, i)`` centred at ``origin + ((i + 1/2), (j + 1/2)) *
    cell_size``; outside the grid the concentration is 0).  One :meth:`advance` tick of ``tick_s`` seconds advects it with the
    plume's wind plus ``eddy_gain * eddies`` (semi-Lagrangian, any displacement), diffuses it (``diffusivity``), holds the source
    cells at their peak (``max`` with the source map), and then moves the wind one Ornstein-Uhlenbeck step towards ``mean_wind``
    (``wind_tau``, ``wind_sigma``; counter-based noise from ``seed``, the world's index and the tick).  The model is build-defined
    (the reference ships no plume): its statement is include/nmf.h, its specification in numpy tests/plume_spec.py.

    Args:
        sim: the batch; a world with several flies resolves to ``sim.for_fly(fly_name)``.
        fly_name: the fly whose odor sensor sites :meth:`get_odor_intensities` reads.
        grid: ``(H, W)`` cells, 8..1024 each.  cell_size, origin: the cell's edge and the grid's corner of least ``(x, y)``.
        source: ``(x, y, radius, peak)`` — the cells whose centre lies within ``radius`` of ``(x, y)`` are held at ``peak`` — or an
            explicit ``(H, W)`` source map.
        mean_wind, wind_tau, wind_sigma: the wind process (``wind_sigma=0``: the wind relaxes to ``mean_wind`` and stays).
        diffusivity: ``kappa``; ``kappa * tick_s / cell_size**2`` must not exceed 1/4.
        eddies: optional static ``(H, W, 2)`` velocity field added to every plume's wind, times ``eddy_gain``.
        intensity_scale: factor of every reading.
        per_world: one plume per world (default), or one plume that all worlds smell.
        seed, first_world: the noise stream; plume ``p`` draws as world ``first_world + p`` (the placement of a shard inside a
            larger population, as ``TurningCPG.reset``).

    ``wind`` ``(n_plumes, 2)`` float32 and ``ticks`` ``(n_plumes,)`` int32 are zero-copy views of the device state, writable between
    launches; so are ``buffers`` (the two ``(n_plumes, H, W)`` grids, ping and pong) and ``parity`` (one int32 word on the device:
    the index of the current buffer, which every kernel reads and every tick flips).  Every method is stream-ordered device work on the simulation's stream except :meth:`concentration`, which reads one
    word back; :meth:`advance` and the readings can be captured in a graph and replayed.
    """

    _destroy_entry, _noun, _views = "nmf_plume_destroy", "plume", ("wind", "ticks", "buffers", "parity")

    def __init__(self, sim, fly_name: str, *, grid, cell_size: float, origin=(0.0, 0.0), source, mean_wind=(0.0, 0.0),
                 wind_tau: float = 1.0, wind_sigma: float = 0.0, diffusivity: float = 0.0, tick_s: float = 0.01, eddies=None,
                 eddy_gain: float = 1.0, intensity_scale: float = 1.0, per_world: bool = True, seed: int = 0, first_world: int = 0):
        sim = fly_batch(sim, fly_name, resolve=True)
        self.sim, self.fly_name = sim, fly_name
        seg, rel = site_arrays(sim.world.fly_lookup[fly_name], ODOR_SENSOR_SITES)
        H, W = (int(v) for v in grid)
        self.grid, self.cell_size, self.origin = (H, W), float(cell_size), (float(origin[0]), float(origin[1]))
        self.n_worlds, self.tick_s = int(sim.n_worlds), float(tick_s)
        self.n_plumes = self.n_worlds if per_world else 1
        src = np.asarray(source, dtype=np.float32)
        if src.ndim == 1 and src.size == 4:
            src = self.disc_source((H, W), self.cell_size, self.origin, *(float(v) for v in src))
        if src.shape != (H, W):
            raise ValueError(f"source must be (x, y, radius, peak) or a map of shape {(H, W)}, got shape {src.shape}")
        self.source = np.ascontiguousarray(src, dtype=np.float32)
        self.eddies = None
        if eddies is not None:
            self.eddies = np.ascontiguousarray(eddies, dtype=np.float32)
            if self.eddies.shape != (H, W, 2):
                raise ValueError(f"eddies must have shape {(H, W, 2)}, got {self.eddies.shape}")
        check_params(_PlumeParams, "nmf_plume_params_size", "sensors.py")
        self._params = _PlumeParams(self.n_plumes, H, W, int(first_world), self.cell_size, self.origin[0], self.origin[1], self.tick_s,
                                    float(diffusivity), float(mean_wind[0]), float(mean_wind[1]), float(wind_tau), float(wind_sigma),
                                    float(eddy_gain), float(intensity_scale), int(seed) & 0xFFFFFFFF)
        h = self._create("nmf_plume_create", sim._batch_h, ctypes.byref(self._params), self.source.ctypes.data,
                         None if self.eddies is None else self.eddies.ctypes.data)
        t, dev, field_ptr = sim._torch, sim.device, _native.lib().nmf_plume_field_ptr
        self.wind = _field_view(sim, field_ptr, h, 0, "<f4", (self.n_plumes, 2))
        self.ticks = _field_view(sim, field_ptr, h, 1, "<i4", (self.n_plumes,))
        self.buffers = tuple(_field_view(sim, field_ptr, h, which, "<f4", (self.n_plumes, H, W)) for which in (2, 3))
        self.parity = _field_view(sim, field_ptr, h, 4, "<i4", (1,))
        self._seg, self._rel = t.as_tensor(seg, device=dev), t.as_tensor(rel, device=dev)
        self.out_of_bounds = t.zeros((self.n_worlds,), dtype=t.uint8, device=dev)

    @staticmethod
    def disc_source(grid, cell_size, origin, x, y, radius, peak) -> np.ndarray:
        """``(H, W)`` float32 source map: ``peak`` in the cells whose centre lies within ``radius`` of ``(x, y)``, 0 elsewhere."""
        H, W = grid
        xc = origin[0] + (np.arange(W, dtype=np.float64) + 0.5) * cell_size
        yc = origin[1] + (np.arange(H, dtype=np.float64) + 0.5) * cell_size
        inside = (xc[None, :] - x) ** 2 + (yc[:, None] - y) ** 2 <= radius ** 2
        return np.where(inside, np.float32(peak), np.float32(0)).astype(np.float32)

    # ---- the field
    def advance(self, n_ticks: int = 1) -> None:
        """``n_ticks`` plume ticks of every plume (two launches per tick; no host sync)."""
        _native.check(_native.lib().nmf_plume_advance(self._handle(), int(n_ticks), self.sim._stream()))

    def reset(self, mask=None) -> None:
        """The plumes of ``mask`` (``(n_plumes,)`` bool, numpy or torch; default all) get empty grids, tick 0 and the mean wind;
        the others keep their state."""
        h = self._handle()
        m = reset_mask(mask, self.n_plumes, self.sim)
        _native.check(_native.lib().nmf_plume_reset(h, None if m is None else m.data_ptr(), self.sim._stream()))

    def set_wind(self, wind) -> None:
        """``(2,)`` or ``(n_plumes, 2)``, numpy or torch: copied into :attr:`wind` on the simulation's stream."""
        self._handle()
        t = self.sim._torch
        if not isinstance(wind, t.Tensor):
            wind = t.as_tensor(np.array(wind, dtype=np.float32))
        if tuple(wind.shape) not in ((2,), (self.n_plumes, 2)):
            raise ValueError(f"Expected a wind of shape (2,) or ({self.n_plumes}, 2), but got {tuple(wind.shape)}")
        self.wind.copy_(wind.to(device=self.sim.device, dtype=t.float32).expand(self.n_plumes, 2))

    def concentration(self):
        """The current grids, ``(n_plumes, H, W)`` float32: a zero-copy view of the buffer the parity word names (read back, so
        this waits for the stream).  The next tick makes it the OLD buffer: clone it to keep it."""
        self._handle()
        return self.buffers[int(self.parity.item()) & 1]

    # ---- the readings
    def sample(self, points):
        """Readings at ``points`` ``(n_worlds, n_pts, 2)`` (x, y), numpy or torch -> float32 ``(n_worlds, n_pts)`` on the device;
        sets :attr:`out_of_bounds`."""
        h = self._handle()
        t = self.sim._torch
        pts = t.as_tensor(points).to(device=self.sim.device, dtype=t.float32).contiguous()
        if pts.ndim != 3 or pts.shape[0] != self.n_worlds or pts.shape[2] != 2 or pts.shape[1] < 1:
            raise ValueError(f"Expected points of shape ({self.n_worlds}, n_pts, 2), but got {tuple(pts.shape)}")
        out = t.empty((self.n_worlds, int(pts.shape[1])), dtype=t.float32, device=self.sim.device)
        _native.check(_native.lib().nmf_plume_sample_points(h, pts.data_ptr(), int(pts.shape[1]), out.data_ptr(),
                                                            self.out_of_bounds.data_ptr(), self.sim._stream()))
        return out

    def get_odor_intensities(self, out=None):
        """float32 ``(n_worlds, 1, 4)`` at the four odor sensor sites (the layout of :meth:`OdorSensors.get_odor_intensities`
        with one odor dimension) from the poses of the last step; sets :attr:`out_of_bounds`.  ``out``: a tensor to fill."""
        h = self._handle()
        t = self.sim._torch
        if out is None:
            out = t.empty((self.n_worlds, 1, 4), dtype=t.float32, device=self.sim.device)
        elif (tuple(out.shape) != (self.n_worlds, 1, 4) or out.dtype != t.float32 or not out.is_contiguous()
              or out.device != t.device(self.sim.device)):
            raise ValueError(f"out must be a contiguous float32 tensor of shape ({self.n_worlds}, 1, 4) on {self.sim.device}")
        _native.check(_native.lib().nmf_plume_sample_sites(h, self._seg.data_ptr(), self._rel.data_ptr(), 4, out.data_ptr(),
                                                           self.out_of_bounds.data_ptr(), self.sim._stream()))
        return out


class _OdometryParams(ctypes.Structure):
    """``nmf_odometry_params`` of include/nmf.h."""

    _fields_ = [("window", ctypes.c_int32), ("root_seg", ctypes.c_int32), ("tip_seg", ctypes.c_int32 * 6),
                ("contact_force_threshold", ctypes.c_float * 6)]


class PathIntegrator(NativeHandle):
    """Path integration on the GPU (``nmf_odometry_*``): the fly's heading and position estimated from proprioception alone, from
    how far each leg's tip travels relative to the body while the leg is on the ground.

    Build-defined (the reference ships no path integration), in the form of flygym 1.x's path-integration task; the statement of
    the model is include/nmf.h (``nmf_odometry_update``), its specification in numpy tests/odometry_spec.py.  One :meth:`update`
    per control tick, from the batch's ``seg_xpos`` / ``seg_xquat`` / ``sensordata`` as they stand when it starts::

        x_l = (tip_l - root) . xhat                       (xhat: the root segment's x axis; float32)
        c_l = found_l > 0 and (thr_l == 0 or |F_l| > thr_l)
        total_l += x_l(previous update) - x_l             while the leg is on the ground in both updates
        win_l = total_l - total_l(``window`` updates ago)
        dh = (heading_bias + sum_l heading_coef_l win_l) / window,  dd = (disp_bias + sum_l disp_coef_l win_l) / window
        heading <- wrap(heading + dh);  position <- position + dd (cos heading, sin heading)        once ``window`` updates are in
        home = -R(heading)^T position                     (the way back to the estimate's origin, in the body frame)

    The first update after a reset only primes the tip coordinates; the estimates stand still for the first ``window`` updates,
    as flygym 1.x's.  A pose that is not finite stays in that world's state until the world is reset.

    Args:
        sim: the batch; for a world with several flies ``sim.for_fly(fly_name)``.
        fly_name: the fly whose legs are read.
        window: updates a stride window spans (1..4096).
        contact_force_thresholds: per leg position ``(f, m, h)``, in the contact sensors' force unit; 0 counts every contact.
        coefficients: 14 values in the device's order — ``heading_coef[6]``, ``disp_coef[6]`` (legs in ``LEGS`` order),
            ``heading_bias``, ``disp_bias`` —, e.g. from :meth:`calibrate`; default zeros.

    ``stride_total`` and ``window_strides`` ``(n, 6)``, ``heading`` ``(n,)``, ``position`` and ``home`` ``(n, 2)`` float64,
    ``count`` ``(n,)`` int32 and ``coefficients`` ``(14,)`` float64 (shared by all worlds) are zero-copy views of the device state,
    writable between launches.  Every method is stream-ordered device work on the simulation's stream; :meth:`update` is one
    launch and can be captured in a graph after the tick's last step.  Close the integrator before its simulation.
    """

    _destroy_entry, _noun = "nmf_odometry_destroy", "integrator"
    _views = ("stride_total", "window_strides", "heading", "position", "home", "count", "coefficients")

    def __init__(self, sim, fly_name: str, *, window: int, contact_force_thresholds=(0.0, 0.0, 0.0), coefficients=None):
        sim = fly_batch(sim, fly_name, resolve=False)
        if fly_name not in sim.world.fly_lookup:
            raise ValueError(f"no fly named {fly_name!r} in this simulation ({', '.join(sim.world.fly_lookup)})")
        if len(contact_force_thresholds) != 3:
            raise ValueError(f"contact_force_thresholds takes one value for each of 'f', 'm', 'h', got {contact_force_thresholds!r}")
        self.sim, self.fly_name = sim, fly_name
        self.n_worlds, self.window = int(sim.n_worlds), int(window)
        self.root_seg, self.tip_seg = leg_segments(sim.world.fly_lookup[fly_name], LEGS)
        by_pos = dict(zip("fmh", (float(v) for v in contact_force_thresholds)))
        self.contact_force_thresholds = np.array([by_pos[leg[1]] for leg in LEGS], dtype=np.float32)
        coef = None
        if coefficients is not None:
            coef = np.ascontiguousarray(coefficients, dtype=np.float64).reshape(-1)
            if coef.size != 14:
                raise ValueError(f"coefficients takes 14 values (heading_coef[6], disp_coef[6], heading_bias, disp_bias), got {coef.size}")
        check_params(_OdometryParams, "nmf_odometry_params_size", "sensors.py")
        self._params = _OdometryParams(self.window, self.root_seg, (ctypes.c_int32 * 6)(*self.tip_seg.tolist()),
                                       (ctypes.c_float * 6)(*self.contact_force_thresholds.tolist()))
        h = self._create("nmf_odometry_create", sim._batch_h, ctypes.byref(self._params), None if coef is None else coef.ctypes.data)
        view = lambda which, typestr="<f8", shape=None: _field_view(sim, _native.lib().nmf_odometry_field_ptr, h, which, typestr, shape)
        self.stride_total, self.window_strides = view(0), view(1)
        self.heading, self.position, self.home = view(2).reshape(self.n_worlds), view(3), view(4)
        self.count = view(5, "<i4").reshape(self.n_worlds)
        self.coefficients = view(6, shape=(14,))

    # ---- the estimate
    def update(self) -> None:
        """One update of every world from the batch's current pose and sensor outputs (one launch; no host sync)."""
        _native.check(_native.lib().nmf_odometry_update(self._handle(), self.sim._stream()))

    def reset(self, mask=None, pose=None) -> None:
        """The worlds of ``mask`` (``(n_worlds,)`` bool, numpy or torch; default all) forget their strides and start again, priming
        included, from ``pose`` (``(n_worlds, 3)`` x, y, heading, numpy or torch; default zeros; the rows of the other worlds are
        not read); the others keep their state."""
        h = self._handle()
        t = self.sim._torch
        m, p = reset_mask(mask, self.n_worlds, self.sim), None
        if pose is not None:
            p = t.as_tensor(pose)
            if tuple(p.shape) != (self.n_worlds, 3):
                raise ValueError(f"Expected a pose of shape ({self.n_worlds}, 3), but got {tuple(p.shape)}")
            p = p.to(device=self.sim.device, dtype=t.float64).contiguous()
        _native.check(_native.lib().nmf_odometry_reset(h, None if m is None else m.data_ptr(), None if p is None else p.data_ptr(),
                                                       self.sim._stream()))

    def set_coefficients(self, heading_coef, disp_coef, heading_bias: float = 0.0, disp_bias: float = 0.0) -> None:
        """Six heading and six displacement coefficients (legs in ``LEGS`` order) and the two biases: copied into
        :attr:`coefficients` on the simulation's stream."""
        self._handle()
        coef = np.concatenate([np.asarray(heading_coef, dtype=np.float64).reshape(-1), np.asarray(disp_coef, dtype=np.float64).reshape(-1),
                               [float(heading_bias), float(disp_bias)]])
        if coef.size != 14:
            raise ValueError("heading_coef and disp_coef take six values each")
        if not np.isfinite(coef).all():
            raise ValueError("the coefficients must be finite")
        self.coefficients.copy_(self.sim._torch.as_tensor(coef).to(self.sim.device))

    def true_pose(self):
        """``(n_worlds, 3)`` float64 on the device: x, y and heading (the direction of the x axis in the ground plane) of the root
        segment, from the poses of the last step: what the estimate is compared with and calibrated against."""
        self._handle()
        t = self.sim._torch
        xpos = self.sim.field("seg_xpos").reshape(self.n_worlds, -1, 3)[:, self.root_seg].to(t.float64)
        qw, qx, qy, qz = self.sim.field("seg_xquat").reshape(self.n_worlds, -1, 4)[:, self.root_seg].to(t.float64).unbind(dim=1)
        heading = t.atan2(2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qy * qy + qz * qz))
        return t.stack([xpos[:, 0], xpos[:, 1], heading], dim=1)

    @staticmethod
    def calibrate(window_strides_trace, pose_trace, window: int):
        """Least-squares coefficients from a recorded walk: ``window_strides_trace`` ``(T, n, 6)`` (:attr:`window_strides` after
        every update) and ``pose_trace`` ``(T, n, 3)`` (:meth:`true_pose` at the same instants).  For every tick ``k >= window`` the
        targets are the heading change ``wrap(h_k - h_{k - window})`` and the distance ``|p_k - p_{k - window}|`` over the window;
        the model has flygym 1.x's structure — the heading change from the three left-minus-right differences of the pairs' window
        strides plus a bias, the distance from the three left-plus-right sums plus a bias —, solved with ``numpy.linalg.lstsq``.
        Returns ``(coefficients (14,) float64 in the device's order, r2_heading, r2_displacement)``."""
        win = np.asarray(window_strides_trace, dtype=np.float64)
        pose = np.asarray(pose_trace, dtype=np.float64)
        W = int(window)
        if win.ndim != 3 or win.shape[2] != 6 or pose.shape != win.shape[:2] + (3,):
            raise ValueError(f"Expected traces of shape (T, n, 6) and (T, n, 3), but got {win.shape} and {pose.shape}")
        if W < 1 or win.shape[0] <= W:
            raise ValueError(f"the traces must be longer than the window ({W} updates), got {win.shape[0]}")
        dh = pose[W:, :, 2] - pose[:-W, :, 2]
        dh = dh - 2.0 * np.pi * np.rint(dh / (2.0 * np.pi))
        dd = np.linalg.norm(pose[W:, :, :2] - pose[:-W, :, :2], axis=-1)
        x = win[W:]
        ones = np.ones(x.shape[:2] + (1,))
        A_h = np.concatenate([x[..., :3] - x[..., 3:], ones], axis=-1).reshape(-1, 4)
        A_d = np.concatenate([x[..., :3] + x[..., 3:], ones], axis=-1).reshape(-1, 4)

        def fit(A, y):
            sol = np.linalg.lstsq(A, y, rcond=None)[0]
            ss = float(((y - y.mean()) ** 2).sum())
            return sol, (1.0 - float(((y - A @ sol) ** 2).sum()) / ss if ss > 0 else 1.0)

        a, r2_h = fit(A_h, dh.reshape(-1))
        b, r2_d = fit(A_d, dd.reshape(-1))
        return np.concatenate([a[:3], -a[:3], b[:3], b[:3], [a[3], b[3]]]), r2_h, r2_d


class _MotionParams(ctypes.Structure):
    """``nmf_motion_params`` of include/nmf.h."""

    _fields_ = [("a_fast", ctypes.c_float), ("a_slow", ctypes.c_float), ("gain", ctypes.c_float), ("delta", ctypes.c_float),
                ("base", ctypes.c_float), ("drive_min", ctypes.c_float), ("drive_max", ctypes.c_float), ("front_edge", ctypes.c_int32 * 2)]


class MotionDetectors(NativeHandle):
    """Motion vision on the GPU (``nmf_motion_*``, ``csrc/nmf_motion.hip``): how the image of each eye moves, and an optomotor
    drive that turns the fly with the panorama so that it holds its course.

    Build-defined (the reference ships no vision processing) and pinned by nothing; the statement of the model is include/nmf.h
    (``nmf_motion_update``), its specification in numpy tests/motion_spec.py.  One :meth:`update` per control tick, from the
    ommatidia readings of both eyes (``EyeRenderer.render_into``)::

        x_i = the reading of ommatidium i;  a world's first update starts from fast_i = slow_i = x_i
        fast_i += a_fast (x_i - fast_i);  slow_i += a_slow (x_i - slow_i);  hp_i = x_i - slow_i     (a = 1 - exp(-dt / tau))
        d_k = fast_a hp_b - hp_a fast_b                           per pair k = (a, b) of neighbouring ommatidia
        H = mean_k d_k wx_k,  V = mean_k d_k wy_k                 per eye ((wx, wy): the unit vector from a to b in the image);
                                                                  each term clamped to +-4 and rounded to 2^-16, summed as integers
        ftb = -H where the image's last column faces forward (``front_edge``), else H       (the flow from front to back)
        rotation = ftb_left - ftb_right   (positive: the panorama turns counter-clockwise about the fly);  translation = their sum
        r = gain rotation;  q = r / (1 + |r|);  o_left = 1 - delta max(q, 0);  o_right = 1 - delta max(-q, 0)
        drive[side] = clip(base[side] o_side, drive_min, drive_max)                         (side 0 = left, as ``TurningCPG.drive``)

    so the side the panorama drifts towards is slowed and the fly turns with it.

    Args:
        sim: the batch; a world with several flies resolves to ``sim.for_fly(fly_name)``.
        fly_name: the fly whose eyes are read.
        dt: the control tick, seconds between two updates.
        retina: the retina whose readings :meth:`update` takes (default: the default :class:`Retina`); at most 1024 ommatidia.
        pairs: ``(pairs (P, 2) int, weights (P, 2) float)`` instead of ``retina.motion_pairs()``; at most 3072 pairs.
        tau_fast, tau_slow: time constants of the two low-pass filters, seconds.
        gain: the rotation at which a side is slowed by ``delta / 2`` is ``1 / gain``.  The default of 320 puts that point at the
            rotation signal the curving open-loop gait itself produces over a checker ground (about 3e-3): chosen from the sweep
            of closed-loop walks recorded in profiles/motion_summary.md.
        delta: the largest share a side is slowed by; 0 switches the reflex off (the drive is ``base``).
        base: the drive without rotation (or pass a tensor to :meth:`update`).

    ``flow`` ``(n, 2, 2)`` (H, V per eye), ``rotation`` and ``translation`` ``(n,)``, ``drive`` ``(n, 2)`` float32, ``sums``
    ``(n, 2, 2)`` int32 (the integer flow sums), the filter states ``fast`` and ``slow`` ``(n, 2, n_omm)`` float32 and ``fresh``
    ``(n,)`` uint8 are zero-copy views of the handle's device memory, allocated once.  Every method is stream-ordered device work on
    the simulation's stream; :meth:`update` is one launch and can be captured in a graph.  Close it before its simulation.
    """

    _destroy_entry, _noun = "nmf_motion_destroy", "motion detector"
    _views = ("fast", "slow", "sums", "flow", "rotation", "translation", "drive", "fresh")

    def __init__(self, sim, fly_name: str, *, dt: float, retina=None, pairs=None, tau_fast: float = 0.035, tau_slow: float = 0.15,
                 gain: float = 320.0, delta: float = 0.8, base: float = 1.0, drive_min: float = 0.2, drive_max: float = 1.2):
        from .controllers import eye_front_edges

        sim = fly_batch(sim, fly_name, resolve=True)
        if fly_name not in sim.world.fly_lookup:
            raise ValueError(f"no fly named {fly_name!r} in this simulation ({', '.join(sim.world.fly_lookup)})")
        if not (dt > 0 and tau_fast > 0 and tau_slow > 0):
            raise ValueError(f"dt, tau_fast and tau_slow must be positive, got {dt!r}, {tau_fast!r}, {tau_slow!r}")
        self.sim, self.fly_name = sim, fly_name
        self.retina = retina or Retina()
        self.n_worlds, self.n_omm = int(sim.n_worlds), int(self.retina.num_ommatidia)
        if self.n_omm > MAX_STEERING_OMMATIDIA:
            raise ValueError(f"a retina of {self.n_omm} ommatidia exceeds the motion kernel's {MAX_STEERING_OMMATIDIA}")
        pr, wt = self.retina.motion_pairs() if pairs is None else pairs
        pr, wt = np.asarray(pr), np.asarray(wt)
        if pr.ndim != 2 or pr.shape[1] != 2 or wt.shape != pr.shape or not np.issubdtype(pr.dtype, np.integer):
            raise ValueError(f"pairs takes (pairs (P, 2) int, weights (P, 2) float), got {pr.shape} {pr.dtype} and {wt.shape} {wt.dtype}")
        if pr.shape[0] > MAX_MOTION_PAIRS:
            raise ValueError(f"{pr.shape[0]} pairs exceed the motion kernel's {MAX_MOTION_PAIRS}")
        if pr.size and (pr.min() < 0 or pr.max() >= self.n_omm):
            raise ValueError(f"a pair index lies outside the retina's {self.n_omm} ommatidia")
        if (pr[:, 0] == pr[:, 1]).any():
            raise ValueError("a pair joins an ommatidium to itself (a == b)")
        self.pairs = np.ascontiguousarray(pr, dtype=np.int32)
        self.weights = np.ascontiguousarray(wt, dtype=np.float32)
        self.n_pairs = int(self.pairs.shape[0])
        self.dt, self.front_edge = float(dt), eye_front_edges()
        self.a_fast = np.float32(1.0 - np.exp(-np.float64(dt) / np.float64(tau_fast)))
        self.a_slow = np.float32(1.0 - np.exp(-np.float64(dt) / np.float64(tau_slow)))
        check_params(_MotionParams, "nmf_motion_params_size", "sensors.py")
        self._params = _MotionParams(float(self.a_fast), float(self.a_slow), float(gain), float(delta), float(base), float(drive_min),
                                     float(drive_max), (ctypes.c_int32 * 2)(*self.front_edge))
        h = self._create("nmf_motion_create", sim._batch_h, ctypes.byref(self._params), self.pairs.ctypes.data if self.n_pairs else None,
                         self.weights.ctypes.data if self.n_pairs else None, self.n_pairs, self.n_omm)
        n = self.n_worlds
        view = lambda which, shape, typestr="<f4": _field_view(sim, _native.lib().nmf_motion_field_ptr, h, which, typestr, shape)
        self.fast, self.slow = view(0, (n, 2, self.n_omm)), view(1, (n, 2, self.n_omm))
        self.sums, self.flow = view(2, (n, 2, 2), "<i4"), view(3, (n, 2, 2))
        self.rotation, self.translation = view(4, (n,)), view(5, (n,))
        self.drive, self.fresh = view(6, (n, 2)), view(7, (n,), "|u1")

    def _checked(self, name, x, shape):
        t = self.sim._torch
        if (not isinstance(x, t.Tensor) or tuple(x.shape) != shape or x.dtype != t.float32 or x.device != self.sim.device
                or not x.is_contiguous()):
            got = f"{tuple(x.shape)} {x.dtype} on {x.device}" if isinstance(x, t.Tensor) else type(x).__name__
            raise ValueError(f"{name} must be a contiguous float32 tensor of shape {shape} on {self.sim.device}, got {got}")
        return x

    def update(self, omm, base=None, out=None):
        """One update from ``omm`` ``(n_worlds, 2, num_ommatidia, 2)`` (float32, contiguous, on the simulation's device): one kernel
        launch on the simulation's stream, no allocation — capturable.  Advances :attr:`fast` and :attr:`slow`, writes
        :attr:`sums`, :attr:`flow`, :attr:`rotation` and :attr:`translation`, and the drive into ``out`` ``(n_worlds, 2)`` (for
        example ``cpg.drive``) or into :attr:`drive`; returns the drive tensor.  ``base`` ``(n_worlds, 2)`` (for example
        ``SensorySteering.drive``) takes the place of the scalar parameter ``base``."""
        h, n = self._handle(), self.n_worlds
        self._checked("omm", omm, (n, 2, self.n_omm, 2))
        if base is not None:
            self._checked("base", base, (n, 2))
        drive = self.drive if out is None else self._checked("out", out, (n, 2))
        _native.check(_native.lib().nmf_motion_update(h, omm.data_ptr(), None if base is None else base.data_ptr(), drive.data_ptr(),
                                                      self.sim._stream()))
        return drive

    def reset(self, mask=None) -> None:
        """The worlds of ``mask`` (``(n_worlds,)`` bool, numpy or torch; default all) forget their filters: their next update starts
        from its readings, as a first update does.  The others keep their state."""
        h = self._handle()
        m = reset_mask(mask, self.n_worlds, self.sim)
        _native.check(_native.lib().nmf_motion_reset(h, None if m is None else m.data_ptr(), self.sim._stream()))


@dataclass
class VisualNetwork:
    """A retinotopic network for :class:`RetinotopicNetwork`, by name: ``types`` the cell types in the order of the views; ``tau``
    (seconds, every type), ``bias``, ``in_w`` (a pair: the weights of the two reading channels) and ``steer_w`` per type name
    (missing: 0); ``edges`` a list of ``(post, pre, {tap: weight})`` with ``tap`` a row of the neighbour table
    (:meth:`Retina.hex_neighbours`).  The taps of an edge are taken in the dict's order, the edges into a type in the list's."""

    types: tuple
    tau: dict
    bias: dict = field(default_factory=dict)
    in_w: dict = field(default_factory=dict)
    steer_w: dict = field(default_factory=dict)
    edges: list = field(default_factory=list)


@dataclass
class FlatNetwork:
    """A network for :class:`RetinotopicNetwork` by index, as ``nmf_visnet_create`` takes it — for networks a program builds:
    ``types`` the names, ``tau``, ``bias``, ``steer_w`` ``(C,)`` and ``in_w`` ``(C, 2)`` arrays, ``edges`` ``(E, 2)`` int (post,
    pre), ``taps`` ``(K, 2)`` int (edge, tap) in any order — the taps of one edge keep their order among themselves, a tap may
    repeat — and ``tap_w`` ``(K,)``."""

    types: tuple
    tau: np.ndarray
    bias: np.ndarray
    in_w: np.ndarray
    steer_w: np.ndarray
    edges: np.ndarray
    taps: np.ndarray
    tap_w: np.ndarray


def _flatten_arrays(net: FlatNetwork, dt: float, substeps: int):
    names = tuple(net.types)
    C = len(names)
    tau = np.asarray(net.tau, dtype=np.float64).reshape(-1)
    edges, taps = np.asarray(net.edges).reshape(-1, 2), np.asarray(net.taps).reshape(-1, 2)
    tap_w = np.asarray(net.tap_w, dtype=np.float32).reshape(-1)
    columns = [np.asarray(net.bias, dtype=np.float32).reshape(-1), *np.asarray(net.in_w, dtype=np.float32).reshape(-1, 2).T,
               np.asarray(net.steer_w, dtype=np.float32).reshape(-1)]
    if C < 1 or tau.shape != (C,) or any(col.shape != (C,) for col in columns) or len(tap_w) != len(taps):
        raise ValueError(f"a flat network of {C} types needs tau, bias and steer_w of shape ({C},), in_w ({C}, 2) and a weight per tap")
    if not (np.issubdtype(edges.dtype, np.integer) or edges.size == 0) or not (np.issubdtype(taps.dtype, np.integer) or taps.size == 0):
        raise ValueError("edges and taps hold integer indices")
    if edges.size and (edges.min() < 0 or edges.max() >= C):
        raise ValueError(f"an edge names a type outside 0..{C - 1}")
    if taps.size and (taps[:, 0].min() < 0 or taps[:, 0].max() >= len(edges)):
        raise ValueError(f"a tap belongs to an edge outside 0..{len(edges) - 1}")
    if not (dt > 0 and (tau > 0).all()):
        raise ValueError(f"dt and every tau must be positive, got dt = {dt!r}, tau = {tau.tolist()}")
    a = (1.0 - np.exp(-np.float64(dt) / (int(substeps) * tau))).astype(np.float32)
    types = np.ascontiguousarray(np.stack([columns[0], columns[1], columns[2], a, columns[3]], axis=-1), dtype=np.float32)
    return names, types, np.ascontiguousarray(edges, dtype=np.int32), np.ascontiguousarray(taps, dtype=np.int32), np.ascontiguousarray(tap_w)


def flatten_network(network, dt: float, substeps: int = 1):
    """``network`` (a :class:`VisualNetwork` or a dict of its fields) as the arrays of ``nmf_visnet_create``: ``(names, types
    (C, 5) float32 — bias, in_w[0], in_w[1], a, steer_w — edges (E, 2) int32 (post, pre), taps (K, 2) int32 (edge, tap), tap_w
    (K,) float32)`` with ``a = float32(1 - exp(-dt / (substeps tau)))`` computed in float64."""
    if isinstance(network, FlatNetwork):
        return _flatten_arrays(network, dt, substeps)
    net = VisualNetwork(**network) if isinstance(network, dict) else network
    names = tuple(net.types)
    if len(set(names)) != len(names) or not names:
        raise ValueError("a network needs at least one cell type, each named once")
    index = {name: c for c, name in enumerate(names)}
    for label, table in (("tau", net.tau), ("bias", net.bias), ("in_w", net.in_w), ("steer_w", net.steer_w)):
        unknown = [k for k in table if k not in index]
        if unknown:
            raise ValueError(f"{label} names the unknown cell type {unknown[0]!r}")
    missing = [name for name in names if name not in net.tau]
    if missing:
        raise ValueError(f"cell type {missing[0]!r} has no tau")
    tau = np.array([net.tau[name] for name in names], dtype=np.float64)
    if not (dt > 0 and (tau > 0).all()):
        raise ValueError(f"dt and every tau must be positive, got dt = {dt!r}, tau = {tau.tolist()}")
    types = np.zeros((len(names), 5), dtype=np.float32)
    types[:, 0] = [net.bias.get(name, 0.0) for name in names]
    types[:, 1:3] = [net.in_w.get(name, (0.0, 0.0)) for name in names]
    types[:, 3] = (1.0 - np.exp(-np.float64(dt) / (int(substeps) * tau))).astype(np.float32)
    types[:, 4] = [net.steer_w.get(name, 0.0) for name in names]
    edges, taps, tap_w = [], [], []
    for e, (post, pre, kernel) in enumerate(net.edges):
        if post not in index or pre not in index:
            raise ValueError(f"edge {e} = ({post!r}, {pre!r}) names an unknown cell type")
        edges.append((index[post], index[pre]))
        for tap, weight in kernel.items():
            taps.append((e, int(tap)))
            tap_w.append(weight)
    return (names, types, np.array(edges, dtype=np.int32).reshape(-1, 2), np.array(taps, dtype=np.int32).reshape(-1, 2),
            np.array(tap_w, dtype=np.float32))


MOTION_DIRECTIONS = {"ftb": (1.0, 0.0), "btf": (-1.0, 0.0), "down": (0.0, 1.0), "up": (0.0, -1.0)}


def motion_pathway(offsets=None) -> VisualNetwork:
    """The build-defined default network of :class:`RetinotopicNetwork`: an elementary-motion-detector pathway of 15 cell types
    per eye.  Pinned by nothing; the values below come from the grating runs of tests/test_visnet_cpu.py.

    ``Lm``  (tau 200 ms, in_w (1, 1)): the local mean luminance.
    ``On``  (tau 5 ms, in_w (1, 1), -1 ``Lm`` at tap 0) and ``Off`` (tau 5 ms, in_w (-1, -1), +1 ``Lm``): the rectified brightening
            and darkening of a cell against its mean.
    ``OnF`` (tau 8 ms) and ``OnD`` (tau 60 ms), each +1 ``On`` at tap 0; ``OffF`` and ``OffD`` likewise: a fast and a delayed copy.
    ``T4ftb``, ``T4btf``, ``T4down``, ``T4up`` (tau 10 ms, bias -0.05): the ON cells that prefer motion along +x, -x, +y, -y of the
            lattice; ``T5...`` the OFF ones.  Each sums +1 of its pathway's fast type at tap 0, +1.5 of the delayed type spread
            over the distance-1 taps on the side the motion comes from (tap ``t`` in proportion to how far ``offsets[t]`` lies
            along that direction) and -1.5 of the delayed type spread likewise over the taps on the side it goes to.
    ``steer_w``: +1 for the ``ftb`` types and -1 for the ``btf`` types.  With the class's default tables +x of the lattice runs from
            front to back across either eye, so the signal is the front-to-back motion of the left eye minus the right eye's: the
            rotation of the panorama, positive counter-clockwise, as ``MotionDetectors.rotation``.

    ``offsets``: the lattice vectors of the distance-1 taps, rows 1..6 of ``Retina.hex_neighbours(...)[1]`` (default: the default
    retina's)."""
    off = np.asarray(Retina().hex_neighbours(1)[1] if offsets is None else offsets, dtype=np.float64)[:7]
    if off.shape != (7, 2):
        raise ValueError(f"offsets must hold the cell itself and its six distance-1 taps, got shape {off.shape}")
    pitch = np.hypot(off[1:, 0], off[1:, 1]).mean()
    types = ["Lm", "On", "Off", "OnF", "OnD", "OffF", "OffD"]
    tau = dict(Lm=0.2, On=0.005, Off=0.005, OnF=0.008, OnD=0.06, OffF=0.008, OffD=0.06)
    in_w = dict(Lm=(1.0, 1.0), On=(1.0, 1.0), Off=(-1.0, -1.0))
    edges = [("On", "Lm", {0: -1.0}), ("Off", "Lm", {0: 1.0}), ("OnF", "On", {0: 1.0}), ("OnD", "On", {0: 1.0}),
             ("OffF", "Off", {0: 1.0}), ("OffD", "Off", {0: 1.0})]
    bias, steer_w = {}, {}
    for cell, path in (("T4", "On"), ("T5", "Off")):
        for name, u in MOTION_DIRECTIONS.items():
            along = off @ np.asarray(u) / pitch                                    # how far each tap lies along the motion
            behind, ahead = {}, {}
            for t in range(1, 7):
                if along[t] < -0.25:
                    behind[t] = -along[t]
                elif along[t] > 0.25:
                    ahead[t] = along[t]
            kind = cell + name
            types.append(kind)
            tau[kind], bias[kind] = 0.01, -0.05
            edges.append((kind, path + "F", {0: 1.0}))
            edges.append((kind, path + "D", {**{t: 1.5 * w / sum(behind.values()) for t, w in behind.items()},
                                             **{t: -1.5 * w / sum(ahead.values()) for t, w in ahead.items()}}))
            if name in ("ftb", "btf"):
                steer_w[kind] = 1.0 if name == "ftb" else -1.0
    return VisualNetwork(types=tuple(types), tau=tau, bias=bias, in_w=in_w, steer_w=steer_w, edges=edges)


def eye_tables(retina, rings: int = 2, front_edge=None):
    """``(neighbours (2, T, n_omm) int32, offsets (T, 2) float64)``: ``retina.hex_neighbours(rings)`` per eye, with the rows of an
    eye whose image has its LAST column facing forward (``front_edge[eye]`` = 1, ``controllers.eye_front_edges``) exchanged so
    that row ``t`` is the tap at ``offsets[t]`` mirrored in x.  Lattice +x then runs from front to back across either eye, and a
    cell type means the same direction about the fly in both.  Needs a lattice that its mirror image maps onto itself."""
    from .controllers import eye_front_edges

    front = eye_front_edges() if front_edge is None else tuple(front_edge)
    table, offsets = retina.hex_neighbours(rings)
    pitch = float(np.hypot(offsets[1:, 0], offsets[1:, 1]).min()) if len(offsets) > 1 else 1.0
    mirrored = offsets * np.array([-1.0, 1.0])
    gap = np.hypot(mirrored[:, None, 0] - offsets[None, :, 0], mirrored[:, None, 1] - offsets[None, :, 1]) / pitch
    swap = gap.argmin(axis=1)
    if (gap[np.arange(len(offsets)), swap] > 0.1).any():
        raise ValueError("the retina's lattice is not its own mirror image in x: pass neighbours of shape (2, T, n_omm)")
    return np.stack([table[swap] if front[eye] else table for eye in range(2)]).astype(np.int32), offsets


class _VisnetParams(ctypes.Structure):
    """``nmf_visnet_params`` of include/nmf.h."""

    _fields_ = [("n_types", ctypes.c_int32), ("n_omm", ctypes.c_int32), ("n_table", ctypes.c_int32), ("n_edges", ctypes.c_int32),
                ("n_taps", ctypes.c_int32), ("substeps", ctypes.c_int32), ("gain", ctypes.c_float), ("delta", ctypes.c_float),
                ("base", ctypes.c_float), ("drive_min", ctypes.c_float), ("drive_max", ctypes.c_float)]


class RetinotopicNetwork(NativeHandle):
    """A retinotopic visual network on the GPU (``nmf_visnet_*``, ``csrc/nmf_visnet.hip``): cell types that are layers of one cell
    per ommatidium, joined by small convolution kernels on the retina's hexagonal lattice and integrated as a leaky recurrent
    system, in the manner of Lappalainen et al. 2024 — the kind of network flygym 1.x's "advanced vision" task reads.  The pooled
    activity of the types, not the image, steers the ``TurningCPG``.

    Build-defined (the reference ships no vision processing) and pinned by nothing; the statement of the model is include/nmf.h
    (``nmf_visnet_update``), its specification in numpy tests/visnet_spec.py, which the kernel equals bit for bit.  One
    :meth:`update` per control tick, from the ommatidia readings of both eyes (``EyeRenderer.render_into``); per eye, ``substeps``
    times with the same readings ``x0_i, x1_i`` (the two channels of ommatidium ``i``)::

        r[c][i] = max(v[c][i], 0)                                            of the old state of every type
        s = bias_c + in_w[c][0] x0_i + in_w[c][1] x1_i + sum over the taps (pre, t, w) into c of  w r[pre][neighbours[t][i]]
        v[c][i] += a_c (s - v[c][i])                                         a_c = 1 - exp(-dt / (substeps tau_c))
    then
        pooled[c] = mean_i min(r[c][i], 4)                                   each term rounded to 2^-16, summed as integers
        signal = sum_c steer_w_c (pooled[left][c] - pooled[right][c])
        g = gain signal;  q = g / (1 + |g|);  o_left = 1 - delta max(q, 0);  o_right = 1 - delta max(-q, 0)
        drive[side] = clip(base[side] o_side, drive_min, drive_max)          (side 0 = left, as ``TurningCPG.drive``)

    a tap on a missing neighbour reads 0, and a world's first update starts from ``v[c][i] = bias_c``.

    Args:
        sim: the batch; a world with several flies resolves to ``sim.for_fly(fly_name)``.
        fly_name: the fly whose eyes are read.
        network: a :class:`VisualNetwork` (or a dict of its fields) or a :class:`FlatNetwork`; :func:`motion_pathway` is the build-defined default.  At most
            32 types, 24576 cells (types x ommatidia), 512 edges and 4096 taps.
        dt: the control tick, seconds between two updates.
        retina: the retina whose readings :meth:`update` takes (default: the default :class:`Retina`); at most 1024 ommatidia.
        neighbours: the neighbour table, ``(T, n_omm)`` for both eyes or ``(2, T, n_omm)`` per eye, ``T`` in 1..19, entries in
            -1..n_omm-1.  Default: :func:`eye_tables` of ``retina`` — the left eye's lattice mirrored, so that +x of the lattice
            runs from front to back across both eyes — with as many rings (0, 1 or 2: 1, 7 or 19 rows) as the network's taps reach.
        substeps: 1..8 repetitions of the rule per update.
        gain: the signal at which a side is slowed by ``delta / 2`` is ``1 / gain``.  The default of 10 is not tuned in closed
            loop: a full-field grating of contrast 0.4 drifting at 2 Hz gives ``motion_pathway`` a signal of 0.21.
        delta: the largest share a side is slowed by; 0 switches the steering off (the drive is ``base``).
        base: the drive without a signal (or pass a tensor to :meth:`update`).

    ``v`` ``(n, 2, C, n_omm)``, ``pooled`` ``(n, 2, C)``, ``signal`` ``(n,)``, ``drive`` ``(n, 2)`` float32, ``sums`` ``(n, 2, C)``
    int32 and ``fresh`` ``(n, 2)`` uint8 are zero-copy views of the handle's device memory, allocated once; ``type_names`` names
    the ``C`` axis.  Every method is stream-ordered device work on the simulation's stream; :meth:`update` is two launches, allocates
    nothing and can be captured in a graph.  Close it before its simulation.
    """

    _destroy_entry, _noun = "nmf_visnet_destroy", "visual network"
    _views = ("v", "pooled", "sums", "signal", "drive", "fresh")

    def __init__(self, sim, fly_name: str, network, *, dt: float, retina=None, neighbours=None, substeps: int = 1, gain: float = 10.0,
                 delta: float = 0.8, base: float = 1.0, drive_min: float = 0.2, drive_max: float = 1.2):
        sim = fly_batch(sim, fly_name, resolve=True)
        if fly_name not in sim.world.fly_lookup:
            raise ValueError(f"no fly named {fly_name!r} in this simulation ({', '.join(sim.world.fly_lookup)})")
        if int(substeps) != substeps or not 1 <= substeps <= MAX_VISNET_SUBSTEPS:
            raise ValueError(f"substeps must be in 1..{MAX_VISNET_SUBSTEPS}, got {substeps!r}")
        self.sim, self.fly_name = sim, fly_name
        self.retina = retina or Retina()
        self.n_worlds, self.n_omm = int(sim.n_worlds), int(self.retina.num_ommatidia)
        if self.n_omm > MAX_STEERING_OMMATIDIA:
            raise ValueError(f"a retina of {self.n_omm} ommatidia exceeds the network kernel's {MAX_STEERING_OMMATIDIA}")
        self.dt, self.substeps = float(dt), int(substeps)
        self.type_names, self.types, self.edges, self.taps, self.tap_w = flatten_network(network, self.dt, self.substeps)
        C = self.n_types = len(self.type_names)
        if C > MAX_VISNET_TYPES or C * self.n_omm > MAX_VISNET_CELLS:
            raise ValueError(f"{C} types x {self.n_omm} ommatidia exceed the network kernel's {MAX_VISNET_TYPES} types or {MAX_VISNET_CELLS} cells")
        if len(self.edges) > MAX_VISNET_EDGES or len(self.taps) > MAX_VISNET_TAPS:
            raise ValueError(f"{len(self.edges)} edges and {len(self.taps)} taps exceed the network kernel's {MAX_VISNET_EDGES} edges or {MAX_VISNET_TAPS} taps")
        if neighbours is None:                               # the smallest table that holds every tap the network reads
            reach = int(self.taps[:, 1].max()) if len(self.taps) else 0
            nb = eye_tables(self.retina, 0 if reach == 0 else 1 if reach < 7 else 2)[0]
        else:
            nb = np.asarray(neighbours)
        if nb.ndim == 2:
            nb = np.stack([nb, nb])
        if nb.ndim != 3 or nb.shape[0] != 2 or not 1 <= nb.shape[1] <= MAX_VISNET_TABLE or nb.shape[2] != self.n_omm or not np.issubdtype(nb.dtype, np.integer):
            raise ValueError(f"neighbours takes an int table of shape (T, {self.n_omm}) or (2, T, {self.n_omm}) with T in 1..{MAX_VISNET_TABLE}, got {nb.shape} {nb.dtype}")
        if nb.min() < -1 or nb.max() >= self.n_omm:
            raise ValueError(f"a neighbour lies outside -1..{self.n_omm - 1}")
        self.neighbours = np.ascontiguousarray(nb, dtype=np.int32)
        if len(self.taps) and (self.taps[:, 1].min() < 0 or self.taps[:, 1].max() >= nb.shape[1]):
            raise ValueError(f"a tap reads a row outside the neighbour table's {nb.shape[1]}")
        if not np.isfinite(self.types).all() or not np.isfinite(self.tap_w).all():
            raise ValueError("a bias, weight or coefficient of the network is not finite")
        check_params(_VisnetParams, "nmf_visnet_params_size", "sensors.py")
        self._params = _VisnetParams(C, self.n_omm, int(nb.shape[1]), len(self.edges), len(self.taps), self.substeps, float(gain),
                                     float(delta), float(base), float(drive_min), float(drive_max))
        h = self._create("nmf_visnet_create", sim._batch_h, ctypes.byref(self._params), self.types.ctypes.data, self.neighbours.ctypes.data,
                         self.edges.ctypes.data if len(self.edges) else None, self.taps.ctypes.data if len(self.taps) else None,
                         self.tap_w.ctypes.data if len(self.taps) else None)
        n = self.n_worlds
        view = lambda which, shape, typestr="<f4": _field_view(sim, _native.lib().nmf_visnet_field_ptr, h, which, typestr, shape)
        self.v, self.pooled, self.sums = view(0, (n, 2, C, self.n_omm)), view(1, (n, 2, C)), view(2, (n, 2, C), "<i4")
        self.signal, self.drive, self.fresh = view(3, (n,)), view(4, (n, 2)), view(5, (n, 2), "|u1")

    _checked = MotionDetectors._checked

    def update(self, omm, base=None, out=None):
        """One update from ``omm`` ``(n_worlds, 2, num_ommatidia, 2)`` (float32, contiguous, on the simulation's device): two kernel
        launches on the simulation's stream, no allocation — capturable.  Advances :attr:`v`, writes :attr:`sums`, :attr:`pooled`
        and :attr:`signal`, and the drive into ``out`` ``(n_worlds, 2)`` (for example ``cpg.drive``) or into :attr:`drive`; returns
        the drive tensor.  ``base`` ``(n_worlds, 2)`` (for example ``MotionDetectors.drive``) takes the place of the scalar
        parameter ``base``."""
        h, n = self._handle(), self.n_worlds
        self._checked("omm", omm, (n, 2, self.n_omm, 2))
        if base is not None:
            self._checked("base", base, (n, 2))
        drive = self.drive if out is None else self._checked("out", out, (n, 2))
        _native.check(_native.lib().nmf_visnet_update(h, omm.data_ptr(), None if base is None else base.data_ptr(), drive.data_ptr(),
                                                      self.sim._stream()))
        return drive

    def reset(self, mask=None) -> None:
        """The worlds of ``mask`` (``(n_worlds,)`` bool, numpy or torch; default all) forget their state: their next update starts
        from ``v = bias``, as a first update does.  The others keep theirs."""
        h = self._handle()
        m = reset_mask(mask, self.n_worlds, self.sim)
        _native.check(_native.lib().nmf_visnet_reset(h, None if m is None else m.data_ptr(), self.sim._stream()))
