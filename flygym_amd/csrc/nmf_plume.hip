// nmf_plume.hip — advected odor plumes on the device (gfx950): flygym_amd.sensors.OdorPlume.
//
// No reference counterpart (the snapshot holds no plume code and no plume data; flygym 1.x replayed one recording of an offline
// fluid simulation to one fly): build-defined; the specification in numpy is tests/plume_spec.py.  A plume is a
// float32 concentration grid c[H][W] over the ground plane, cell (j, i) centred at (x0 + (i + 1/2) h, y0 + (j + 1/2) h); cells
// outside the grid read as 0 everywhere (clean air in, odor out).  One tick, every cell from the old grid:
//
//   v = w + eddy_gain E[j][i]                                        (w: the plume's wind; E: optional static eddies, shared)
//   d = vx r, k = floor(d), f = d - k;  (l, g) likewise along y      (r = dt / h: index units, any displacement, no CFL clamp)
//   adv = (1 - g) ((1 - f) c[j-l][i-k] + f c[j-l][i-k-1]) + g ((1 - f) c[j-l-1][i-k] + f c[j-l-1][i-k-1])
//   dif = D (c[j][i-1] + c[j][i+1] + c[j-1][i] + c[j+1][i] - 4 c[j][i])           (D = kappa dt / h^2 <= 1/4)
//   c_new[j][i] = max(adv + dif, S[j][i])                                             (S: the source map, shared)
//
// then the wind's Ornstein-Uhlenbeck step w <- w + a (mean - w) + b xi with counter-based noise (plume_noise), and tick <- tick + 1.
//
// Two grids per plume, ping and pong.  WHICH one is current is a word in device memory (parity): the tick kernel reads it and
// writes the other grid, the wind kernel flips it.  No host-side pointer swap, so a captured launch sequence replays correctly
// any number of times.
//
// Tick kernel: one lane per cell, a workgroup per (plume, tile of 64 x 4 cells); a wave is 64 consecutive cells of one row, so
// the centre load and the store are whole coalesced segments, and the eight neighbour / upstream reads are the same segments
// shifted: they come from L1 / L2 (a 128 x 256 grid is 128 KiB; the source map and the eddies are shared by all plumes).  No LDS,
// no atomics: every cell is written once by one lane from the old grid alone, so results are bitwise reproducible.  Two
// restructurings that cut the load instructions per cell from ten to four (a lane per four cells with 16-byte loads, with and
// without divergence at the borders) were measured and bought 17 % without eddies and nothing with them — the tick is not bound
// by its load instructions —, so the plain form stays: profiles/plume_summary.md.
#include "nmf_device.h"

namespace nmf {

constexpr int kPlumeTileW = 64, kPlumeTileH = 4;
constexpr int kPlumeThreads = kPlumeTileW * kPlumeTileH;
constexpr float kPlumeMaxShift = 4096.f;     // whole-cell displacements are clamped here before they become integers: the grid is
                                             // at most 1024 cells wide, so every clamped displacement reads outside it (zeros) anyway

struct PlumeArgs {
  int n_plumes, H, W, first_world;
  float x0, y0, h, scale;                    // origin, cell size, intensity_scale (the readings)
  float r, D, eddy_gain;                     // r = dt / h, D = kappa dt / h^2
  float a, b, mean_x, mean_y;                // a = dt / tau, b = sigma sqrt(dt), the mean wind
  unsigned int seed;
};

// c[j][i], 0 outside the grid
__device__ __forceinline__ float plume_cell(const float* c, int H, int W, int j, int i) {
  return ((unsigned)j < (unsigned)H && (unsigned)i < (unsigned)W) ? c[j * W + i] : 0.f;
}

// The bilinear blend both the advection and the readings use: rows j and j + dj, columns i and i + di, weights (1 - g, g) x
// (1 - f, f), every operation rounded as written (no contraction: the specification's float32 flavour, bit for bit)
__device__ __forceinline__ float plume_blend(const float* c, int H, int W, int j, int i, int dj, int di, float g, float f) {
#pragma clang fp contract(off) reassociate(off)
  const float c00 = plume_cell(c, H, W, j, i), c01 = plume_cell(c, H, W, j, i + di);
  const float c10 = plume_cell(c, H, W, j + dj, i), c11 = plume_cell(c, H, W, j + dj, i + di);
  return (1.f - g) * ((1.f - f) * c00 + f * c01) + g * ((1.f - f) * c10 + f * c11);
}

__global__ void __launch_bounds__(kPlumeThreads)
nmf_plume_tick_kernel(PlumeArgs A, const int* __restrict__ parity, const float* __restrict__ wind, const float* __restrict__ eddies,
                      const float* __restrict__ source, float* grid0, float* grid1) {
#pragma clang fp contract(off) reassociate(off)
  const int tiles_x = (A.W + kPlumeTileW - 1) / kPlumeTileW, tiles = tiles_x * ((A.H + kPlumeTileH - 1) / kPlumeTileH);
  const int p = blockIdx.x / tiles, t = blockIdx.x - p * tiles;
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int i = tx * kPlumeTileW + (threadIdx.x & (kPlumeTileW - 1)), j = ty * kPlumeTileH + threadIdx.x / kPlumeTileW;
  if (i >= A.W || j >= A.H) return;
  const int par = *parity & 1, cell = j * A.W + i;
  const size_t base = (size_t)p * (size_t)(A.H * A.W);
  const float* c = (par ? grid1 : grid0) + base;
  float* out = (par ? grid0 : grid1) + base;
  float vx = wind[2 * p], vy = wind[2 * p + 1];
  if (eddies) {
    const float2 e = reinterpret_cast<const float2*>(eddies)[cell];
    vx = vx + A.eddy_gain * e.x;
    vy = vy + A.eddy_gain * e.y;
  }
  const float dx = vx * A.r, dy = vy * A.r;
  const float kf = floorf(dx), lf = floorf(dy);
  // (fminf / fmaxf drop a NaN: a wind the caller wrote as NaN or infinity must not index outside the grid)
  const int k = (int)fminf(fmaxf(kf, -kPlumeMaxShift), kPlumeMaxShift), l = (int)fminf(fmaxf(lf, -kPlumeMaxShift), kPlumeMaxShift);
  const float adv = plume_blend(c, A.H, A.W, j - l, i - k, -1, -1, dy - lf, dx - kf);
  const float ring = (plume_cell(c, A.H, A.W, j, i - 1) + plume_cell(c, A.H, A.W, j, i + 1))
                   + (plume_cell(c, A.H, A.W, j - 1, i) + plume_cell(c, A.H, A.W, j + 1, i));
  out[cell] = fmaxf(adv + A.D * (ring - 4.f * c[cell]), source[cell]);
}

__device__ __forceinline__ unsigned int plume_hash(unsigned int x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}

// xi = ((u0 + u1) + (u2 + u3) - 2) sqrt(3), u_m = (hash(key ^ (m0 + m) 0xC2B2AE35) >> 8) 2^-24: mean 0, variance 1, |xi| <= 2 sqrt(3).
// Rounded as written (no contraction; the file is compiled without reassociation, see nmf_capi.hip).
__device__ __forceinline__ float plume_noise(unsigned int key, unsigned int m0) {
#pragma clang fp contract(off) reassociate(off)
  float u[4];
#pragma unroll
  for (unsigned int m = 0; m < 4; ++m) u[m] = (float)(plume_hash(key ^ ((m0 + m) * 0xC2B2AE35u)) >> 8) * 0x1p-24f;
  return (((u[0] + u[1]) + (u[2] + u[3])) - 2.f) * 1.7320508075688772f;
}

// After the grids: one lane per plume steps its wind and its tick counter; the first lane flips the parity word.
__global__ void nmf_plume_wind_kernel(PlumeArgs A, int* __restrict__ parity, float* __restrict__ wind, unsigned int* __restrict__ ticks) {
#pragma clang fp contract(off) reassociate(off)
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p == 0) *parity = (*parity & 1) ^ 1;
  if (p >= A.n_plumes) return;
  const unsigned int tick = ticks[p];
  const unsigned int key = A.seed ^ ((unsigned int)(A.first_world + p) * 0x9E3779B9u) ^ (tick * 0x85EBCA6Bu);
  const float wx = wind[2 * p], wy = wind[2 * p + 1];
  wind[2 * p] = (wx + A.a * (A.mean_x - wx)) + A.b * plume_noise(key, 0u);
  wind[2 * p + 1] = (wy + A.a * (A.mean_y - wy)) + A.b * plume_noise(key, 4u);
  ticks[p] = tick + 1u;
}

// Both grids zero, tick 0 and the mean wind for the plumes of the mask (all when mask is null); one lane per cell
__global__ void nmf_plume_reset_kernel(PlumeArgs A, const uint8_t* __restrict__ mask, float* __restrict__ grid0, float* __restrict__ grid1,
                                       float* __restrict__ wind, unsigned int* __restrict__ ticks) {
  const size_t cells = (size_t)(A.H * A.W), idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= cells * (size_t)A.n_plumes) return;
  const size_t p = idx / cells;
  if (mask && !mask[p]) return;
  grid0[idx] = 0.f;
  grid1[idx] = 0.f;
  if (idx == p * cells) { wind[2 * p] = A.mean_x; wind[2 * p + 1] = A.mean_y; ticks[p] = 0u; }
}

// The reading at (x, y): the current grid interpolated between cell centres, u = (x - x0) / h - 1/2 (the division correctly
// rounded: the specification's), times intensity_scale.  oob: (u, v) outside [-1/2, W - 1/2] x [-1/2, H - 1/2], or not a number.
__device__ __forceinline__ float plume_read(const PlumeArgs& A, const float* c, float x, float y, bool& oob) {
  const float u = (float)__ddiv_rn((double)(x - A.x0), (double)A.h) - 0.5f, v = (float)__ddiv_rn((double)(y - A.y0), (double)A.h) - 0.5f;
  oob = !(u >= -0.5f && u <= (float)A.W - 0.5f && v >= -0.5f && v <= (float)A.H - 0.5f);
  if (!(u > -1.f && u < (float)A.W && v > -1.f && v < (float)A.H)) return 0.f;      // all four cells outside
  const float fu = floorf(u), fv = floorf(v);
  return plume_blend(c, A.H, A.W, (int)fv, (int)fu, 1, 1, v - fv, u - fu) * A.scale;
}

// The current grid of world w's plume (one shared plume: n_plumes == 1)
__device__ __forceinline__ const float* plume_of_world(const PlumeArgs& A, const int* parity, const float* grid0, const float* grid1, int w) {
  return ((*parity & 1) ? grid1 : grid0) + (size_t)(A.n_plumes == 1 ? 0 : w) * (size_t)(A.H * A.W);
}

// The world's flag: any lane of its wave read out of bounds
__device__ __forceinline__ void plume_flag(uint8_t* oob, int w, bool any) {
  const bool wave_any = __ballot(any) != 0ull;
  if ((threadIdx.x & (kWave - 1)) == 0) oob[w] = wave_any ? 1 : 0;
}

constexpr int kPlumeSampleThreads = 256;     // a wave per world, its lanes over the world's points

// out[w][k] = the reading at points[w][k] = (x, y)
__global__ void __launch_bounds__(kPlumeSampleThreads)
nmf_plume_sample_points_kernel(PlumeArgs A, int n_worlds, const int* __restrict__ parity, const float* __restrict__ grid0,
                               const float* __restrict__ grid1, const float* __restrict__ points, int n_pts, float* __restrict__ out,
                               uint8_t* __restrict__ oob) {
  const int w = blockIdx.x * (kPlumeSampleThreads / kWave) + threadIdx.x / kWave;
  if (w >= n_worlds) return;
  const float* c = plume_of_world(A, parity, grid0, grid1, w);
  bool any = false;
  for (int k = threadIdx.x & (kWave - 1); k < n_pts; k += kWave) {
    const size_t at = (size_t)w * (size_t)n_pts + (size_t)k;
    bool o;
    out[at] = plume_read(A, c, points[2 * at], points[2 * at + 1], o);
    any |= o;
  }
  plume_flag(oob, w, any);
}

// out[w][k] = the reading at the x, y of seg_xpos + R(seg_xquat) rel of sensor k's parent segment (as nmf_odor_kernel places it)
__global__ void __launch_bounds__(kPlumeSampleThreads)
nmf_plume_sample_sites_kernel(PlumeArgs A, int n_worlds, const int* __restrict__ parity, const float* __restrict__ grid0,
                              const float* __restrict__ grid1, const float* __restrict__ seg_xpos, const float* __restrict__ seg_xquat,
                              int nseg, const int* __restrict__ sensor_seg, const float* __restrict__ sensor_rel, int n_sensor,
                              float* __restrict__ out, uint8_t* __restrict__ oob) {
  const int w = blockIdx.x * (kPlumeSampleThreads / kWave) + threadIdx.x / kWave;
  if (w >= n_worlds) return;
  const float* c = plume_of_world(A, parity, grid0, grid1, w);
  bool any = false;
  for (int k = threadIdx.x & (kWave - 1); k < n_sensor; k += kWave) {
    const int sg = min(max(sensor_seg[k], 0), nseg - 1);      // (a segment index the caller got wrong must not read outside the pose)
    const float* xp = seg_xpos + ((size_t)w * nseg + sg) * 3;
    float R[9];
    qmat(R, ldq(seg_xquat + ((size_t)w * nseg + sg) * 4));
    const V3 pos = ld3(xp) + mat_vec(R, ld3(sensor_rel + 3 * k));
    bool o;
    out[(size_t)w * (size_t)n_sensor + (size_t)k] = plume_read(A, c, pos.x, pos.y, o);
    any |= o;
  }
  plume_flag(oob, w, any);
}

}  // namespace nmf
