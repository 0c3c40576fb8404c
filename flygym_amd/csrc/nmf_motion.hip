// nmf_motion.hip — motion vision on the device (gfx950): flygym_amd.sensors.MotionDetectors.
//
// No reference counterpart (the snapshot holds no vision processing): build-defined; the statement of the model is
// include/nmf.h (nmf_motion_update), its specification in numpy tests/motion_spec.py.  One launch per control tick turns the
// ommatidia readings of both eyes into the wide-field flow of each eye and an optomotor drive for the CPG:
//
//   per eye and ommatidium: x = omm[i][0] + omm[i][1];  a fresh world starts from fast = slow = x
//            fast += a_fast (x - fast);  slow += a_slow (x - slow);  hp = x - slow
//   per eye and pair k = (a, b, wx, wy) of neighbouring ommatidia:  d = fast_a hp_b - hp_a fast_b      (Hassenstein-Reichardt)
//            Sx += (int) rint(clamp(d wx, -4, 4) 2^16),  Sy likewise with wy                           (int32)
//            H = Sx / (2^16 P), V = Sy / (2^16 P), or 0 without pairs
//   ftb_e = front_edge[e] ? -H_e : H_e;  rotation = ftb_0 - ftb_1;  translation = ftb_0 + ftb_1        (a zero is +0)
//   r = gain rotation;  q = r / (1 + |r|);  o_left = 1 - delta max(q, 0), o_right = 1 - delta max(-q, 0)
//   drive[side] = clamp(base[side] o_side, drive_min, drive_max)
//
// The sums are integers of terms rounded to 2^-16 before they are added, so the flow does not depend on the order of the
// reduction (|term| <= 2^18 and P <= 3072 < 2^12: a sum stays below 2^30 whatever the readings, a NaN term counting as -4); the
// quotients are correctly rounded double divisions (nmf_exact.h) rounded once to float; the float32 rule is compiled without
// contraction and reassociation.  Kernel and specification therefore agree bit for bit.
//
// One wave per (world, eye), two worlds per workgroup.  Part 1: the lanes stride over the eye's ommatidia — the reading pair is one
// 8-byte load, the two filter states one 4-byte load and one 4-byte store each (a wave: contiguous 512- and 256-byte segments) —
// and leave (fast, hp) as one 8-byte cell of the wave's LDS slice (1024 x 8 B; exactly 32 KiB a workgroup, so five workgroups =
// 20 waves fit a CU's 160 KiB).  The slice of the state belongs to this wave alone, so it is updated in place.  Part 2, after the
// barrier: the lanes stride over the pair list (16 B a pair, shared by all worlds: L2), read both ends from LDS (ds_read_b64,
// random banks) and accumulate the two sums; a DPP ladder (wave_reduce_bits) adds them across the wave, which leaves them in
// cell 0 of its slice.  Part 3, after a second barrier: one lane per world reads the four sums of its two eyes from LDS,
// evaluates the rule and clears the world's fresh byte (both eyes read it in part 1).  The fresh bytes live in device memory: a
// masked reset works and a captured update replays.  No atomics; every pointer is a kernel argument or lives in the handle; the
// launch allocates nothing.
#include "nmf.h"
#include "nmf_device.h"
#include "nmf_exact.h"

namespace nmf {

constexpr int kMotionMaxPairs = 3072;
constexpr int kMotionThreads = 256;                              // four waves: two worlds x two eyes
constexpr int kMotionWorlds = kMotionThreads / (2 * kWave);      // worlds per workgroup
constexpr float kMotionClamp = 4.f, kMotionScale = 65536.f;      // a term is clamped to +-4 and rounded to 2^-16

struct MotionArgs {
  nmf_motion_params p;
  int n_worlds, n_omm, n_pairs;
  double den;                                  // 2^16 n_pairs, exact
};

// the shared pair list and the per-world state and outputs of a handle
struct MotionPtrs {
  const int4* pairs;                           // [n_pairs] (a, b, bits of wx, bits of wy)
  float* fast; float* slow;                    // [n_worlds][2][n_omm]
  uint8_t* fresh;                              // [n_worlds]
  int* sums;                                   // [n_worlds][2][2] Sx, Sy per eye
  float* flow;                                 // [n_worlds][2][2] H, V per eye
  float* rotation; float* translation;         // [n_worlds]
};

// state + a (x - state), each operation rounded
__device__ __forceinline__ float motion_lowpass(float state, float a, float x) {
#pragma clang fp contract(off) reassociate(off)
  const float d = x - state;
  const float m = a * d;
  return state + m;
}

// The two fixed-point terms of one pair from its ends' (fast, hp)
__device__ __forceinline__ void motion_pair_terms(float2 ca, float2 cb, float wx, float wy, int& tx, int& ty) {
#pragma clang fp contract(off) reassociate(off)
  const float p0 = ca.x * cb.y, p1 = ca.y * cb.x;
  const float d = p0 - p1;
  const float dx = d * wx, dy = d * wy;
  tx = (int)rintf(fminf(fmaxf(dx, -kMotionClamp), kMotionClamp) * kMotionScale);
  ty = (int)rintf(fminf(fmaxf(dy, -kMotionClamp), kMotionClamp) * kMotionScale);
}

// Steps 5 to 7 of one world from the integer sums of its two eyes: s[eye][Sx, Sy]
__device__ __forceinline__ void motion_world(const MotionArgs& A, const MotionPtrs& P, int w, const int (&s)[2][2], const float* __restrict__ base,
                                             float* __restrict__ drive) {
#pragma clang fp contract(off) reassociate(off)
  const nmf_motion_params& p = A.p;
  float hv[2][2];
#pragma unroll
  for (int e = 0; e < 2; ++e)
#pragma unroll
    for (int c = 0; c < 2; ++c) hv[e][c] = A.n_pairs > 0 ? (float)div_rn((double)s[e][c], A.den) : 0.f;
  const float ftb0 = p.front_edge[0] ? -hv[0][0] : hv[0][0], ftb1 = p.front_edge[1] ? -hv[1][0] : hv[1][0];
  const float rotation = plus_zero(ftb0 - ftb1), translation = plus_zero(ftb0 + ftb1);
  const float r = p.gain * rotation;
  const float q = (float)div_rn((double)r, (double)(1.f + fabsf(r)));
  const float o[2] = {1.f - p.delta * fmaxf(q, 0.f), 1.f - p.delta * fmaxf(-q, 0.f)};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    P.sums[(size_t)w * 4 + k] = s[k / 2][k % 2];
    P.flow[(size_t)w * 4 + k] = hv[k / 2][k % 2];
  }
  P.rotation[w] = rotation;
  P.translation[w] = translation;
#pragma unroll
  for (int side = 0; side < 2; ++side) {
    const float b = base ? base[(size_t)w * 2 + side] : p.base;
    drive[(size_t)w * 2 + side] = fminf(fmaxf(b * o[side], p.drive_min), p.drive_max);
  }
  P.fresh[w] = 0;
}

__global__ void __launch_bounds__(kMotionThreads)
nmf_motion_kernel(MotionArgs A, MotionPtrs P, const float2* __restrict__ omm, const float* __restrict__ base, float* __restrict__ drive) {
#pragma clang fp contract(off) reassociate(off)
  // (fast, hp) per ommatidium of the wave's eye; once the wave has its two sums, their bits in cell 0 (exactly 32 KiB in all)
  __shared__ float2 cell[kMotionThreads / kWave][kMaxOmmatidia];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int w = blockIdx.x * kMotionWorlds + wave / 2, eye = wave & 1;
  const bool on = w < A.n_worlds;                                 // (whole waves; the barriers below are reached by every wave)
  if (on) {
    const size_t row = ((size_t)w * 2 + (size_t)eye) * (size_t)A.n_omm;
    const float2* rd = omm + row;
    float* fast = P.fast + row;
    float* slow = P.slow + row;
    const bool fresh = P.fresh[w] != 0;
    const float a_fast = A.p.a_fast, a_slow = A.p.a_slow;
#pragma unroll 4
    for (int i = lane; i < A.n_omm; i += kWave) {
      const float2 r = rd[i];
      const float f0 = fast[i], s0 = slow[i];
      const float x = r.x + r.y;                                  // (one channel is 0: the sum is the reading, exactly)
      const float f = motion_lowpass(fresh ? x : f0, a_fast, x);
      const float s = motion_lowpass(fresh ? x : s0, a_slow, x);
      fast[i] = f;
      slow[i] = s;
      cell[wave][i] = make_float2(f, x - s);
    }
  }
  __syncthreads();
  if (on) {
    auto add = [](int a, int b) { return a + b; };
    int sx = 0, sy = 0;
#pragma unroll 2
    for (int k = lane; k < A.n_pairs; k += kWave) {
      const int4 pr = P.pairs[k];
      int tx, ty;
      motion_pair_terms(cell[wave][pr.x], cell[wave][pr.y], __int_as_float(pr.z), __int_as_float(pr.w), tx, ty);
      sx += tx;
      sy += ty;
    }
    sx = wave_reduce_bits(sx, 0, add);
    sy = wave_reduce_bits(sy, 0, add);
    if (lane == 0) cell[wave][0] = make_float2(__int_as_float(sx), __int_as_float(sy));      // (every lane's reads of the slice are in sx, sy)
  }
  __syncthreads();
  const int ww = blockIdx.x * kMotionWorlds + (int)threadIdx.x;
  if (threadIdx.x < kMotionWorlds && ww < A.n_worlds) {
    const int t = 2 * (int)threadIdx.x;
    const float2 left = cell[t][0], right = cell[t + 1][0];
    const int s[2][2] = {{__float_as_int(left.x), __float_as_int(left.y)}, {__float_as_int(right.x), __float_as_int(right.y)}};
    motion_world(A, P, ww, s, base, drive);
  }
}

// fresh = 1 for the worlds of the mask (all when mask is null): their next update starts the filters from its readings
__global__ void nmf_motion_reset_kernel(int n_worlds, const uint8_t* __restrict__ mask, uint8_t* __restrict__ fresh) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n_worlds) return;
  if (mask && !mask[w]) return;
  fresh[w] = 1;
}

}  // namespace nmf
