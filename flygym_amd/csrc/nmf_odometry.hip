// nmf_odometry.hip — path integration on the device (gfx950): flygym_amd.sensors.PathIntegrator.
//
// No reference counterpart (the snapshot holds no path integration): build-defined in the form of flygym 1.x's path-integration
// task; the statement of the model is include/nmf.h (nmf_odometry_update), its specification in numpy
// tests/odometry_spec.py.  One launch per control tick reads the batch's seg_xpos / seg_xquat / sensordata as they stand when it
// starts and, per world, adds each leg's stance stride (how far its tip moved backwards along the body's x axis while it was on
// the ground in this and the previous tick) to a float64 total, keeps a ring of the last `window` totals, and turns the strides of
// the window into a heading and a displacement increment through 14 shared float64 coefficients:
//
//   x_l = (d . xhat) float32, d = tip_l - root;  c_l = found_l > 0 and (thr_l == 0 or |F_l|^2 > thr_l^2)
//   total_l += (count > 0 and c_l and cprev_l) ? (double)(xprev_l - x_l) : 0
//   win_l = total_l - ring[count mod window][l];  ring[count mod window][l] = total_l
//   dh = (heading_bias + sum_l heading_coef_l win_l) / window, dd likewise;   only once count >= window:
//   heading <- wrap(heading + dh);  position <- position + dd (cos, sin)((float) heading);  home = -R(heading)^T position
//
// One lane per (world, leg): ten worlds in 60 lanes of a wave as in nmf_cpg.hip, four waves per workgroup, so a world's six lanes
// never straddle a wave.  The six-term sums take the legs' win by __shfl from lanes base + j, j = 0..5 in this order for every lane:
// a world's result does not depend on where in the batch it sits.  The ring is [window][n_worlds][6] float64: after a common reset
// every world is at the same slot, and a wave reads and writes one contiguous 480-byte row segment per update; the per-leg state
// arrays ([n_worlds][6]) are contiguous over the wave's lanes likewise.  The pose and sensor reads are strided by the batch's row
// widths (the root's position and quaternion are one broadcast line per world).  count is per world and lives in device memory:
// a masked reset works and a captured update replays correctly.  No LDS, no atomics, no division; all arithmetic is compiled
// without contraction and reassociation, so kernel and specification agree bit for bit up to the sine and cosine (odo_sincos below:
// float64, within 2e-15 of the exact ones).
#include "nmf.h"
#include "nmf_device.h"

namespace nmf {

constexpr int kOdoThreads = 256;
constexpr int kOdoWaveWorlds = 10;                                   // worlds per wave: 60 lanes
constexpr int kOdoWorlds = kOdoWaveWorlds * (kOdoThreads / kWave);   // worlds per workgroup

struct OdoArgs {
  int n_worlds, nseg, root_seg, window;
  int tip_seg[6];
  float thr[6];
  double inv_window;                         // 1.0 / window, the host's float64 quotient
};

// the batch arrays an update reads, the shared coefficients and the per-world state
struct OdoPtrs {
  const float* seg_xpos; const float* seg_xquat; const float* sensordata;
  const double* coef;                        // heading_coef[6], disp_coef[6], heading_bias, disp_bias
  int* count; float* xprev; uint8_t* cprev;
  double* total; double* ring; double* win; double* heading; double* position; double* home;
};

// h - 2 pi rint(h / 2 pi): the product with the reciprocal, the product with 2 pi and the difference each rounded
__device__ __forceinline__ double odo_wrap(double h) {
#pragma clang fp contract(off) reassociate(off)
  constexpr double kTwoPi = 6.283185307179586, kInvTwoPi = 0.15915494309189535;
  const double turns = __builtin_rint(h * kInvTwoPi);
  const double back = kTwoPi * turns;
  return h - back;
}

// Sine and cosine of the float32-rounded heading, evaluated in float64: Cody-Waite reduction to [-pi/4, pi/4] with a two-part pi/2
// whose high part has 33 bits (k pi/2_hi is exact), then the Taylor polynomials to r^15 and r^14 (the first terms left out are
// 5e-17 and 1e-15 at pi/4).  Plain arithmetic, no division, unaffected by the build's approximate-function flag.  The estimates
// are float64 sums of dd times these factors and home multiplies by them once more, so the factors are kept far below the 1e-7
// of the distance that the estimates are held to; the step kernel's float32 sincos_bounded (9.2e-8) is not.
__device__ __forceinline__ void odo_sincos(float heading, double* sn, double* cs) {
#pragma clang fp contract(off) reassociate(off)
  constexpr double kTwoOverPi = 0.63661977236758134308, kPio2Hi = 1.57079632673412561417e+00, kPio2Lo = 6.07710050650619224932e-11;
  constexpr double S1 = -1.0 / 6.0, S2 = 1.0 / 120.0, S3 = -1.0 / 5040.0, S4 = 1.0 / 362880.0, S5 = -1.0 / 39916800.0,
                   S6 = 1.0 / 6227020800.0, S7 = -1.0 / 1307674368000.0;
  constexpr double C1 = -0.5, C2 = 1.0 / 24.0, C3 = -1.0 / 720.0, C4 = 1.0 / 40320.0, C5 = -1.0 / 3628800.0, C6 = 1.0 / 479001600.0,
                   C7 = -1.0 / 87178291200.0;
  const double x = (double)heading;
  const double k = __builtin_rint(x * kTwoOverPi);
  const double r = (x - k * kPio2Hi) - k * kPio2Lo;
  const double z = r * r;
  const double s = r + (r * z) * (S1 + z * (S2 + z * (S3 + z * (S4 + z * (S5 + z * (S6 + z * S7))))));
  const double c = 1.0 + z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * (C6 + z * C7))))));
  const int q = (int)fmin(fmax(k, -1.0e9), 1.0e9) & 3;      // (a heading the caller wrote may be huge: keep the conversion defined)
  const double ss = (q & 1) ? c : s, cc = (q & 1) ? s : c;
  *sn = (q & 2) ? -ss : ss;
  *cs = ((q + 1) & 2) ? -cc : cc;
}

// (-(c px + s py), -(-s px + c py)): the origin of the estimate seen from the body
__device__ __forceinline__ void odo_home(double c, double s, double px, double py, double* out) {
#pragma clang fp contract(off) reassociate(off)
  const double a = c * px, b = s * py, u = s * px, v = c * py;
  out[0] = -(a + b);
  out[1] = -(v - u);
}

__global__ void __launch_bounds__(kOdoThreads)
nmf_odometry_update_kernel(OdoArgs A, OdoPtrs P) {
#pragma clang fp contract(off) reassociate(off)
  const int lane = threadIdx.x & (kWave - 1);
  const int leg = lane % 6, base = lane - leg;
  const int w = (blockIdx.x * (kOdoThreads / kWave) + threadIdx.x / kWave) * kOdoWaveWorlds + lane / 6;
  const bool on = lane < 6 * kOdoWaveWorlds && w < A.n_worlds;   // (the other lanes run along on zeros and store nothing)
  int count = 0;
  double win = 0.0;
  if (on) {
    int tip = A.tip_seg[0];
    float thr = A.thr[0];
#pragma unroll
    for (int j = 1; j < 6; ++j) { tip = leg == j ? A.tip_seg[j] : tip; thr = leg == j ? A.thr[j] : thr; }
    const size_t k = (size_t)w * 6 + (size_t)leg;
    const float* xp = P.seg_xpos + (size_t)w * (size_t)A.nseg * 3;
    const float* rp = xp + 3 * A.root_seg;
    const float* tp = xp + 3 * tip;
    const float* q = P.seg_xquat + ((size_t)w * (size_t)A.nseg + (size_t)A.root_seg) * 4;
    const float qw = q[0], qx = q[1], qy = q[2], qz = q[3];
    const float ax = 1.f - 2.f * (qy * qy + qz * qz), ay = 2.f * (qx * qy + qw * qz), az = 2.f * (qx * qz - qw * qy);
    const float dx = tp[0] - rp[0], dy = tp[1] - rp[1], dz = tp[2] - rp[2];
    const float x = (dx * ax + dy * ay) + dz * az;
    const float4 sd = *reinterpret_cast<const float4*>(P.sensordata + (size_t)w * 96 + 16 * (size_t)leg);   // found, fx, fy, fz
    const float f2 = (sd.y * sd.y + sd.z * sd.z) + sd.w * sd.w;
    const bool c = sd.x > 0.f && (thr == 0.f || f2 > thr * thr);
    count = P.count[w];
    const float xo = P.xprev[k];
    const bool co = P.cprev[k] != 0;
    const double inc = (count > 0 && c && co) ? (double)(xo - x) : 0.0;
    const double tot = P.total[k] + inc;
    int slot = count % A.window;               // (a count the caller wrote below zero must not index outside the ring)
    slot = slot < 0 ? slot + A.window : slot;
    double* cell = P.ring + ((size_t)slot * (size_t)A.n_worlds + (size_t)w) * 6 + (size_t)leg;
    win = tot - *cell;
    *cell = tot;
    P.total[k] = tot;
    P.win[k] = win;
    P.xprev[k] = x;
    P.cprev[k] = c ? 1 : 0;
  }
  // the world's six win, from lanes base + j in the same order for every lane
  double dh = P.coef[12], dd = P.coef[13];
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const double wj = __shfl(win, min(base + j, kWave - 1));
    const double ph = P.coef[j] * wj, pd = P.coef[6 + j] * wj;
    dh = dh + ph;
    dd = dd + pd;
  }
  if (!on || leg != 0) return;
  dh = dh * A.inv_window;
  dd = dd * A.inv_window;
  const bool valid = count >= A.window;
  double h = P.heading[w], px = P.position[2 * (size_t)w], py = P.position[2 * (size_t)w + 1];
  if (valid) h = odo_wrap(h + dh);
  double sn, cs;
  odo_sincos((float)h, &sn, &cs);
  if (valid) {
    const double sx = dd * cs, sy = dd * sn;
    px = px + sx;
    py = py + sy;
  }
  P.heading[w] = h;
  P.position[2 * (size_t)w] = px;
  P.position[2 * (size_t)w + 1] = py;
  odo_home(cs, sn, px, py, P.home + 2 * (size_t)w);
  P.count[w] = (int)((unsigned)count + 1u);
}

// count = 0, totals, window strides and ring rows 0, no previous sample; the estimate starts from pose[w] = (x, y, heading) (zeros
// when pose is null), for the worlds of the mask (all when mask is null).  A 2-D grid: x over (world, leg), y over the ring's
// `window` slots (at most 4096); the threads of slot 0 also clear the rest of the state.
__global__ void nmf_odometry_reset_kernel(OdoArgs A, OdoPtrs P, const uint8_t* __restrict__ mask, const double* __restrict__ pose) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int s = blockIdx.y;
  if (i >= 6 * A.n_worlds || s >= A.window) return;
  const int w = i / 6, leg = i - 6 * w;
  if (mask && !mask[w]) return;
  P.ring[(size_t)s * (size_t)A.n_worlds * 6 + (size_t)i] = 0.0;
  if (s != 0) return;
  P.total[i] = 0.0;
  P.win[i] = 0.0;
  P.xprev[i] = 0.f;
  P.cprev[i] = 0;
  if (leg != 0) return;
  const double px = pose ? pose[3 * (size_t)w] : 0.0, py = pose ? pose[3 * (size_t)w + 1] : 0.0;
  const double h = odo_wrap(pose ? pose[3 * (size_t)w + 2] : 0.0);
  double sn, cs;
  odo_sincos((float)h, &sn, &cs);
  P.count[w] = 0;
  P.heading[w] = h;
  P.position[2 * (size_t)w] = px;
  P.position[2 * (size_t)w + 1] = py;
  odo_home(cs, sn, px, py, P.home + 2 * (size_t)w);
}

}  // namespace nmf
