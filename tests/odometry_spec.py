"""Path integration in numpy: the specification of ``flygym_amd/csrc/nmf_odometry.hip`` (``sensors.PathIntegrator``).  TEST
INFRASTRUCTURE.

Build-defined and pinned by nothing: the reference snapshot holds no path integration.  The form is flygym 1.x's path-integration
task — the strides of the legs over a window predict the change of heading and the distance walked —; the statement of the model is
include/nmf.h (``nmf_odometry_update``).

Float32 arrays where the kernel is float32 (the body-frame coordinate, the force magnitude), float64 where it is float64 (totals,
ring, sums, heading, position), every operation rounded on its own as numpy's arrays give; the sine and cosine are ``np.sin`` /
``np.cos`` of the float32-rounded heading widened to float64, which the kernel's own float64 polynomials approach to 2e-15."""
import numpy as np

f32, f64 = np.float32, np.float64
TWO_PI = f64(6.283185307179586)
INV_TWO_PI = f64(0.15915494309189535)
MAX_WINDOW = 4096


def wrap(h):
    """h - 2 pi rint(h / 2 pi), three roundings."""
    h = np.asarray(h, dtype=f64)
    return h - TWO_PI * np.rint(h * INV_TWO_PI)


def x_axis(quat):
    """(n, 3) float32: the x axis of the frames with quaternions (n, 4) (w, x, y, z), in the kernel's float32 operations."""
    w, x, y, z = np.asarray(quat, dtype=f32).T
    one, two = f32(1), f32(2)
    return np.stack([one - two * (y * y + z * z), two * (x * y + w * z), two * (x * z - w * y)], axis=1).astype(f32)


def fore_aft(seg_xpos, seg_xquat, root_seg, tip_seg):
    """(n, 6) float32: x_l = (tip_l - root) . xhat, summed left to right."""
    n = len(seg_xpos)
    xpos = np.asarray(seg_xpos, dtype=f32).reshape(n, -1, 3)
    quat = np.asarray(seg_xquat, dtype=f32).reshape(n, -1, 4)
    ax = x_axis(quat[:, root_seg])
    d = (xpos[:, np.asarray(tip_seg)] - xpos[:, root_seg][:, None, :]).astype(f32)                 # (n, 6, 3)
    p = (d * ax[:, None, :]).astype(f32)
    return ((p[..., 0] + p[..., 1]).astype(f32) + p[..., 2]).astype(f32)


def contacts(sensordata, thresholds):
    """(n, 6) bool: found_l > 0 and (thr_l == 0 or |F_l|^2 > thr_l^2), in float32."""
    s = np.asarray(sensordata, dtype=f32).reshape(len(sensordata), 6, 16)
    thr = np.asarray(thresholds, dtype=f32).reshape(6)
    f = s[..., 1:4]
    sq = (f * f).astype(f32)
    mag2 = ((sq[..., 0] + sq[..., 1]).astype(f32) + sq[..., 2]).astype(f32)
    return (s[..., 0] > 0) & ((thr == 0) | (mag2 > (thr * thr).astype(f32)))


def trig(heading):
    """(cos, sin) float64 of the float32-rounded heading."""
    h = np.asarray(heading, dtype=f64).astype(f32).astype(f64)
    return np.cos(h), np.sin(h)


def home_vector(position, heading):
    c, s = trig(heading)
    px, py = position[..., 0], position[..., 1]
    return np.stack([-(c * px + s * py), -(-(s * px) + c * py)], axis=-1)


class State:
    """The state of ``n`` worlds, as the handle holds it."""

    def __init__(self, n, window, thresholds=(0,) * 6, coefficients=None):
        assert 1 <= int(window) <= MAX_WINDOW
        self.n, self.window = int(n), int(window)
        self.inv_window = f64(1.0) / f64(self.window)
        self.thr = np.asarray(thresholds, dtype=f32).reshape(6)
        self.coef = np.zeros(14, dtype=f64) if coefficients is None else np.asarray(coefficients, dtype=f64).reshape(14).copy()
        self.count = np.zeros(n, dtype=np.int32)
        self.xprev = np.zeros((n, 6), dtype=f32)
        self.cprev = np.zeros((n, 6), dtype=bool)
        self.total = np.zeros((n, 6), dtype=f64)
        self.ring = np.zeros((self.window, n, 6), dtype=f64)
        self.win = np.zeros((n, 6), dtype=f64)
        self.heading = np.zeros(n, dtype=f64)
        self.position = np.zeros((n, 2), dtype=f64)
        self.home = np.zeros((n, 2), dtype=f64)
        self.dd = np.zeros(n, dtype=f64)              # the last update's displacement increment, 0 where it was not valid
        self.moved = np.zeros(n, dtype=f64)           # sum of |dd| over the valid updates since the world's reset: the tolerance's scale

    def reset(self, mask=None, pose=None):
        m = np.ones(self.n, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
        p = np.zeros((self.n, 3), dtype=f64) if pose is None else np.asarray(pose, dtype=f64)
        self.count[m] = 0
        self.xprev[m] = 0
        self.cprev[m] = False
        self.total[m] = 0
        self.win[m] = 0
        self.ring[:, m] = 0
        self.heading[m] = wrap(p[m, 2])
        self.position[m] = p[m, :2]
        self.home[m] = home_vector(self.position[m], self.heading[m])
        self.dd[m] = 0
        self.moved[m] = 0

    def update_from(self, x, c):
        """One update from the float32 coordinates ``x`` (n, 6) and the contact flags ``c`` (n, 6)."""
        x = np.asarray(x, dtype=f32)
        c = np.asarray(c).astype(bool)
        worlds = np.arange(self.n)
        step = (self.xprev - x).astype(f32).astype(f64)
        inc = np.where((self.count > 0)[:, None] & c & self.cprev, step, f64(0))
        total = self.total + inc
        slot = np.mod(self.count, self.window)
        win = total - self.ring[slot, worlds]
        self.ring[slot, worlds] = total
        valid = self.count >= self.window
        dh = np.full(self.n, self.coef[12], dtype=f64)
        dd = np.full(self.n, self.coef[13], dtype=f64)
        for l in range(6):
            dh = dh + self.coef[l] * win[:, l]
            dd = dd + self.coef[6 + l] * win[:, l]
        dh = dh * self.inv_window
        dd = dd * self.inv_window
        heading = np.where(valid, wrap(self.heading + dh), self.heading)
        cs, sn = trig(heading)
        pos = self.position + np.stack([dd * cs, dd * sn], axis=1)
        self.position = np.where(valid[:, None], pos, self.position)
        self.heading = heading
        self.home = home_vector(self.position, self.heading)
        self.total, self.win = total, win
        self.xprev, self.cprev = x.copy(), c.copy()
        self.count = self.count + np.int32(1)
        self.dd = np.where(valid, dd, f64(0))
        self.moved = self.moved + np.abs(self.dd)

    def update(self, seg_xpos, seg_xquat, sensordata, root_seg, tip_seg):
        """One update from the batch's arrays (n, nseg * 3), (n, nseg * 4) and (n, 96)."""
        self.update_from(fore_aft(seg_xpos, seg_xquat, root_seg, tip_seg), contacts(sensordata, self.thr))
