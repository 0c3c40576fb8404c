// nmf_taxis.hip — sensory steering on the device (gfx950): flygym_amd.controllers.SensorySteering.
//
// No reference counterpart (the snapshot holds no controller and no vision processing): build-defined; the
// statement of the model is include/nmf.h (nmf_taxis_update), its specification in numpy tests/taxis_spec.py.  One launch per
// control tick turns the ommatidia readings of both eyes and the readings of the four odor sites into the CPG's drive:
//
//   per eye: dark_i = omm[i][0] + omm[i][1] < obj_threshold;  cnt = #dark, Sx = sum_dark qx_i, Sy = sum_dark qy_i   (int32)
//            (cy, cx, area) = (Sy / (16 cnt H), Sx / (16 cnt W), cnt / n_omm), or (1/2, 1/2, 0) when nothing is dark
//            dev = front_edge ? 1 - cx : cx;  v = area > area_threshold ? clamp(1 - visual_gain dev, v_min, v_max) : 1
//   odor:    L_d = w_ant I[d][2] + w_palp I[d][0], R_d likewise from I[d][3], I[d][1];  c_d = (L_d - R_d) / (L_d + R_d) or 0
//            b = sum_d g_d c_d;  q = b |b| / (1 + b b);  o_left = 1 - odor_delta max(q, 0), o_right = 1 - odor_delta max(-q, 0)
//   drive[side] = clamp((base v_side) o_side, drive_min, drive_max)
//
// The sums are integers (the centres qx, qy are int16 sixteenths of a pixel), so the features do not depend on the order of the
// reduction; the quotients are correctly rounded double divisions of exact operands, rounded once to float; the float32 rule is
// compiled without contraction and reassociation.  Kernel and specification therefore agree bit for bit.
//
// One wave per world, four worlds per workgroup.  For each eye the lanes stride over the ommatidia: a lane's reading pair is one
// 8-byte load (64 lanes: one 512-byte segment), its centre pair one 4-byte load of a table all worlds share (4 KiB at most: L2).
// Three int32 accumulators per lane, a DPP ladder across the wave (wave_reduce_bits), no LDS, no atomics.  Lane 0 then reads the
// world's n_dims x 4 odor values, evaluates the rule and writes features, bias and drive.  Every pointer is a kernel argument:
// the launch allocates nothing and replays from a captured graph.
#include "nmf.h"
#include "nmf_device.h"
#include "nmf_exact.h"      // div_rn: the correctly rounded double division

namespace nmf {

// (at most kMaxOmmatidia = 1024 ommatidia, nmf_sensors.hip; centres are int16: a sum stays below 2^10 x 2^15 = 2^25)
constexpr int kTaxisMaxDims = 8;
constexpr int kTaxisMaxSide = 2047;          // the int16 range of a centre in sixteenths of a pixel
constexpr int kTaxisThreads = 256;           // a wave per world

struct TaxisArgs {
  nmf_taxis_params p;
  int n_worlds, n_omm, n_dims, H, W;
};

// (cy, cx, area) of one eye from its integer sums
__device__ __forceinline__ void taxis_features(const TaxisArgs& A, int cnt, int sx, int sy, float (&f)[3]) {
  if (cnt == 0) { f[0] = 0.5f; f[1] = 0.5f; f[2] = 0.f; return; }
  f[0] = (float)div_rn((double)sy, (double)(16 * cnt * A.H));
  f[1] = (float)div_rn((double)sx, (double)(16 * cnt * A.W));
  f[2] = (float)div_rn((double)cnt, (double)A.n_omm);
}

// The speed factor of one side from its eye: 1 unless the eye found an object
__device__ __forceinline__ float taxis_visual_speed(const nmf_taxis_params& p, int front_edge, const float (&f)[3]) {
#pragma clang fp contract(off) reassociate(off)
  if (!(f[2] > p.area_threshold)) return 1.f;
  const float dev = front_edge ? 1.f - f[1] : f[1];
  return fminf(fmaxf(1.f - p.visual_gain * dev, p.v_min), p.v_max);
}

// b = sum_d g_d c_d over ascending d, from the world's odor readings I[d][site] (sites: palp L, palp R, antenna L, antenna R)
__device__ __forceinline__ float taxis_odor_bias(const nmf_taxis_params& p, const float* __restrict__ I, const float* __restrict__ gains,
                                                 int n_dims) {
#pragma clang fp contract(off) reassociate(off)
  float b = 0.f;
  for (int d = 0; d < n_dims; ++d) {
    const float4 r = reinterpret_cast<const float4*>(I)[d];
    const float L = p.w_ant * r.z + p.w_palp * r.x, R = p.w_ant * r.w + p.w_palp * r.y;
    const float s = L + R;
    const float c = s > 0.f ? (float)div_rn((double)(L - R), (double)s) : 0.f;
    b = b + gains[d] * c;
  }
  // A sum that starts at +0 is never -0, but the library's -fno-signed-zeros lets the compiler drop the `0 +` of the first term
  // (a negative gain times c = 0 is -0): put the sign right in integer arithmetic, which no floating-point licence touches.
  const unsigned int bits = __float_as_uint(b);
  return __uint_as_float((bits << 1) == 0u ? 0u : bits);
}

__global__ void __launch_bounds__(kTaxisThreads)
nmf_taxis_kernel(TaxisArgs A, const int* __restrict__ centres, const float2* __restrict__ omm, const float* __restrict__ odor,
                 const float* __restrict__ gains, float* __restrict__ features, float* __restrict__ bias, float* __restrict__ drive) {
#pragma clang fp contract(off) reassociate(off)
  const int lane = threadIdx.x & (kWave - 1);
  const int w = blockIdx.x * (kTaxisThreads / kWave) + threadIdx.x / kWave;
  if (w >= A.n_worlds) return;                                 // (whole waves: the ladders below run with every lane)
  const nmf_taxis_params& p = A.p;
  float f[2][3] = {{0.5f, 0.5f, 0.f}, {0.5f, 0.5f, 0.f}};
  if (omm) {
    auto add = [](int a, int b) { return a + b; };
    for (int e = 0; e < 2; ++e) {
      const float2* rd = omm + ((size_t)w * 2 + (size_t)e) * (size_t)A.n_omm;
      int cnt = 0, sx = 0, sy = 0;
#pragma unroll 4
      for (int i = lane; i < A.n_omm; i += kWave) {
        const float2 r = rd[i];
        const int q = centres[i];                              // (x in the low half, y in the high half)
        const bool dark = r.x + r.y < p.obj_threshold;         // (one channel is 0: the sum is the reading, exactly)
        cnt += dark ? 1 : 0;
        sx += dark ? (int)(short)(q & 0xffff) : 0;
        sy += dark ? q >> 16 : 0;
      }
      cnt = wave_reduce_bits(cnt, 0, add);
      sx = wave_reduce_bits(sx, 0, add);
      sy = wave_reduce_bits(sy, 0, add);
      taxis_features(A, cnt, sx, sy, f[e]);
    }
  }
  if (lane != 0) return;
  const float v[2] = {taxis_visual_speed(p, p.front_edge[0], f[0]), taxis_visual_speed(p, p.front_edge[1], f[1])};
  const float b = odor ? taxis_odor_bias(p, odor + (size_t)w * (size_t)(A.n_dims * 4), gains, A.n_dims) : 0.f;
  const float q = (float)div_rn((double)(b * fabsf(b)), (double)(1.f + b * b));
  const float o[2] = {1.f - p.odor_delta * fmaxf(q, 0.f), 1.f - p.odor_delta * fmaxf(-q, 0.f)};
  if (features) {
#pragma unroll
    for (int k = 0; k < 6; ++k) features[(size_t)w * 6 + k] = f[k / 3][k % 3];
  }
  if (bias) bias[w] = b;
#pragma unroll
  for (int s = 0; s < 2; ++s) drive[(size_t)w * 2 + s] = fminf(fmaxf((p.base * v[s]) * o[s], p.drive_min), p.drive_max);
}

}  // namespace nmf
