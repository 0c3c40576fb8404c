"""Sensory steering in numpy: the specification of ``flygym_amd/csrc/nmf_taxis.hip`` (``controllers.SensorySteering``).  TEST
INFRASTRUCTURE.

Build-defined and pinned by nothing: the reference snapshot holds no controller and no vision processing.  The form is flygym 1.x's
two sensorimotor tasks — visual taxis (follow a dark object) and odor taxis — and the default constants are flygym 1.x's as
remembered; every one is a parameter.  The statement of the model is include/nmf.h (``nmf_taxis_update``).

The integer part (which ommatidia are dark, how many, the sums of their centres) is exact; each feature is one float64 division of
exact integers rounded once to float32; everything after is float32 with every operation rounded as written, which numpy's float32
arrays give.  ``np.fmax`` / ``np.fmin`` are the kernel's ``fmaxf`` / ``fminf``."""
import numpy as np

f32 = np.float32

DEFAULTS = dict(obj_threshold=0.15, area_threshold=0.01, visual_gain=3.0, v_min=0.4, v_max=1.2, w_ant=10.0 / 11.0, w_palp=1.0 / 11.0,
                odor_delta=0.8, base=1.0, drive_min=0.2, drive_max=1.2)
MAX_OMMATIDIA, MAX_SIDE, MAX_DIMS = 1024, 2047, 8


def ommatidia_centres(id_map: np.ndarray) -> np.ndarray:
    """float64 (n_omm, 2): the mean (x, y) of the pixel centres (col + 1/2, row + 1/2) of each ommatidium's cell (ids 1..n_omm;
    0 = no ommatidium).  Written per ommatidium, unlike ``Retina.ommatidia_centres``."""
    id_map = np.asarray(id_map)
    out = np.zeros((int(id_map.max()), 2))
    for k in range(out.shape[0]):
        rows, cols = np.nonzero(id_map == k + 1)
        out[k] = (cols.mean() + 0.5, rows.mean() + 0.5)
    return out


def centre_table(centres: np.ndarray) -> np.ndarray:
    """int16 (n_omm, 2): the centres in sixteenths of a pixel."""
    q = np.rint(16.0 * np.asarray(centres, dtype=np.float64))
    assert q.min() >= -32768 and q.max() <= 32767
    return q.astype(np.int16)


def front_edge(eye_cameras: dict) -> tuple:
    """Per eye: 1 when the fly's forward axis (+x of the eye's parent frame) has a positive component along the camera's right
    axis — column 0 of R = Rz(e2) Ry(e1) Rx(e0) — so that the image's last column faces forward; else 0."""
    out = []
    for _, (_, e) in eye_cameras.items():
        cx, sx, cy, sy, cz, sz = np.cos(e[0]), np.sin(e[0]), np.cos(e[1]), np.sin(e[1]), np.cos(e[2]), np.sin(e[2])
        rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
        ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
        rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
        out.append(int((rz @ ry @ rx)[0, 0] > 0))
    return tuple(out)


def features(omm: np.ndarray, table: np.ndarray, height: int, width: int, obj_threshold: float = DEFAULTS["obj_threshold"]) -> np.ndarray:
    """omm (..., n_omm, 2) float32 readings -> (..., 3) float32 (cy, cx, area)."""
    omm = np.asarray(omm, dtype=f32)
    n_omm = omm.shape[-2]
    reading = omm[..., 0] + omm[..., 1]
    dark = reading < f32(obj_threshold)
    q = np.asarray(table, dtype=np.int64)
    cnt = dark.sum(axis=-1).astype(np.int64)
    sx = (dark * q[:, 0]).sum(axis=-1)
    sy = (dark * q[:, 1]).sum(axis=-1)
    some = cnt > 0
    den = np.where(some, cnt, 1)
    out = np.empty(omm.shape[:-2] + (3,), dtype=f32)
    out[..., 0] = np.where(some, (sy.astype(np.float64) / (16 * den * int(height)).astype(np.float64)).astype(f32), f32(0.5))
    out[..., 1] = np.where(some, (sx.astype(np.float64) / (16 * den * int(width)).astype(np.float64)).astype(f32), f32(0.5))
    out[..., 2] = np.where(some, (cnt.astype(np.float64) / np.float64(n_omm)).astype(f32), f32(0))
    return out


def visual_speed(feat: np.ndarray, front, *, area_threshold, visual_gain, v_min, v_max, **_) -> np.ndarray:
    """feat (..., 2, 3) float32 -> (..., 2) float32: each side's speed factor from its eye."""
    feat = np.asarray(feat, dtype=f32)
    cx, area = feat[..., 1], feat[..., 2]
    dev = np.where(np.asarray(front, dtype=bool), f32(1) - cx, cx).astype(f32)
    prod = (f32(visual_gain) * dev).astype(f32)
    v = np.fmin(np.fmax((f32(1) - prod).astype(f32), f32(v_min)), f32(v_max)).astype(f32)
    return np.where(area > f32(area_threshold), v, f32(1)).astype(f32)


def odor_bias(odor: np.ndarray, gains, *, w_ant, w_palp, **_) -> np.ndarray:
    """odor (..., n_dims, 4) float32 (palp L, palp R, antenna L, antenna R) -> (...,) float32: b = sum_d g_d c_d."""
    odor = np.asarray(odor, dtype=f32)
    gains = np.asarray(gains, dtype=f32).reshape(-1)
    assert odor.shape[-2] == gains.size <= MAX_DIMS
    wa, wp = f32(w_ant), f32(w_palp)
    b = np.zeros(odor.shape[:-2], dtype=f32)
    for d in range(gains.size):
        I = odor[..., d, :]
        L = ((wa * I[..., 2]).astype(f32) + (wp * I[..., 0]).astype(f32)).astype(f32)
        R = ((wa * I[..., 3]).astype(f32) + (wp * I[..., 1]).astype(f32)).astype(f32)
        s = (L + R).astype(f32)
        with np.errstate(divide="ignore", invalid="ignore"):
            c = np.where(s > 0, ((L - R).astype(f32) / np.where(s > 0, s, f32(1))).astype(f32), f32(0)).astype(f32)
        b = (b + (gains[d] * c).astype(f32)).astype(f32)
    return b


def squash(b: np.ndarray) -> np.ndarray:
    """q = (b |b|) / (1 + b b): odd, monotone, |q| < 1."""
    b = np.asarray(b, dtype=f32)
    return ((b * np.abs(b)).astype(f32) / (f32(1) + (b * b).astype(f32)).astype(f32)).astype(f32)


def drive_from(v: np.ndarray, b: np.ndarray, *, odor_delta, base, drive_min, drive_max, **_) -> np.ndarray:
    """v (..., 2), b (...,) -> drive (..., 2) float32, side 0 = left."""
    q = squash(b)
    delta = f32(odor_delta)
    o = np.stack([(f32(1) - (delta * np.fmax(q, f32(0))).astype(f32)).astype(f32),
                  (f32(1) - (delta * np.fmax(-q, f32(0))).astype(f32)).astype(f32)], axis=-1)
    raw = ((f32(base) * np.asarray(v, dtype=f32)).astype(f32) * o).astype(f32)
    return np.fmin(np.fmax(raw, f32(drive_min)), f32(drive_max)).astype(f32)


def update(omm=None, odor=None, *, table=None, height=0, width=0, gains=(), front=(1, 0), n_worlds=None, **params):
    """The whole rule: ``(features (n, 2, 3), bias (n,), drive (n, 2))`` float32.  Either input may be absent."""
    p = {**DEFAULTS, **params}
    assert omm is not None or odor is not None
    n = int((omm if omm is not None else odor).shape[0]) if n_worlds is None else n_worlds
    if omm is not None:
        feat = features(omm, table, height, width, p["obj_threshold"])
        v = visual_speed(feat, front, **p)
    else:
        feat = np.tile(np.array([0.5, 0.5, 0.0], dtype=f32), (n, 2, 1))
        v = np.ones((n, 2), dtype=f32)
    b = odor_bias(odor, gains, **p) if odor is not None else np.zeros(n, dtype=f32)
    return feat, b, drive_from(v, b, **p)
