// nmf_navigator.hip — plume navigation on the device (gfx950): flygym_amd.controllers.PlumeNavigator.
//
// No reference counterpart (the snapshot holds no controllers): build-defined and pinned by nothing, in the form of the stochastic
// encounter-driven navigator of Demir et al. 2020 that flygym 1.x steered its plume-tracking task with; the statement
// of the model is include/nmf.h (nmf_navigator_update), its specification in numpy tests/navigator_spec.py.  One launch per control
// tick reads the antennal readings, the wind and the root segment's quaternion as they stand when it starts and, per world, counts
// an odor onset ("encounter") when the antennal sum rises above the threshold, feeds three leaky filters with it, and advances a
// walk / stop / turn state machine whose stop and start rates depend on the first two filters and whose turns are biased upwind by
// the third; the new state picks the drive (left, right) of a TurningCPG from a four-row table.
//
// One lane per world, 256 per workgroup (16 workgroups at 4096 worlds).  The antennae come as the odor dimension's aligned float4,
// the quaternion as one 16-byte load strided by the batch's row, the wind as row w or row 0; the state arrays are contiguous over
// the lanes.  No LDS, no atomics, no division, no transcendental: the host passes the filters' decays.  The three random draws of
// a tick are nmf_plume.hip's counter-based hash of (seed, global world index, tick, draw index 8..10): the tick word lives in
// device memory, so a captured update draws fresh noise on every replay, and a world's stream does not depend on the batch it is
// stepped in.  All arithmetic is compiled without contraction and reassociation and every clamp is a pair of comparisons, so
// kernel and specification agree bit for bit, values that are not finite included (those only ever reach comparisons).
#include "nmf.h"
#include "nmf_device.h"

namespace nmf {

constexpr int kNavThreads = 256;

struct NavArgs {
  nmf_navigator_params p;
  int n_worlds, nseg;
};

// the batch array an update reads and the per-world state
struct NavPtrs {
  const float* seg_xquat;
  int* state; int* remaining; uint8_t* above;
  float* k_stop; float* k_walk; float* freq;
  unsigned int* ticks; int* encounters;
  float* drive;
};

// x < lo ? lo : (x > hi ? hi : x): a NaN passes through both comparisons (numpy's np.where form, not fmin / fmax)
__device__ __forceinline__ float nav_clamp(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

__device__ __forceinline__ float nav_uniform(unsigned int key, unsigned int m) {
  return (float)(plume_hash(key ^ (m * 0xC2B2AE35u)) >> 8) * 0x1p-24f;
}

// the drive row of a state: walk, stop, turn (inner, outer) with the inner side left; a right turn swaps the pair
__device__ __forceinline__ float2 nav_drive(const nmf_navigator_params& p, int state) {
  if (state == NMF_NAV_WALK) return make_float2(p.walk_drive[0], p.walk_drive[1]);
  if (state == NMF_NAV_STOP) return make_float2(p.stop_drive[0], p.stop_drive[1]);
  if (state == NMF_NAV_TURN_RIGHT) return make_float2(p.turn_drive[1], p.turn_drive[0]);
  return make_float2(p.turn_drive[0], p.turn_drive[1]);
}

__global__ void __launch_bounds__(kNavThreads)
nmf_navigator_update_kernel(NavArgs A, NavPtrs P, const float* __restrict__ odor, int n_dims, const float* __restrict__ wind,
                            int wind_rows, float* __restrict__ drive_out) {
#pragma clang fp contract(off) reassociate(off)
  const int w = blockIdx.x * kNavThreads + threadIdx.x;
  if (w >= A.n_worlds) return;
  const nmf_navigator_params& p = A.p;
  const float4 I = *reinterpret_cast<const float4*>(odor + ((size_t)w * (size_t)n_dims + (size_t)p.odor_dim) * 4);   // palps, antennae
  const float4 q = *reinterpret_cast<const float4*>(P.seg_xquat + ((size_t)w * (size_t)A.nseg + (size_t)p.root_seg) * 4);
  const size_t wr = wind_rows == 1 ? 0 : (size_t)w;
  const float wx = wind[2 * wr], wy = wind[2 * wr + 1];
  const int state = P.state[w];
  const unsigned int tick = P.ticks[w];

  // the encounter and the filters
  const float s = I.z + I.w;
  const bool now = s > p.threshold;
  const bool e = now && P.above[w] == 0;
  const float ef = e ? 1.f : 0.f;
  const float k_stop = P.k_stop[w] * p.decay_stop + ef;
  const float k_walk = P.k_walk[w] * p.decay_walk + ef;
  const float freq = P.freq[w] * p.decay_freq + (e ? p.inv_tau_freq : 0.f);

  // which side upwind lies on: the body's x axis (as nmf_odometry.hip) against the wind
  const float qw = q.x, qx = q.y, qy = q.z, qz = q.w;
  const float ax = 1.f - 2.f * (qy * qy + qz * qz), ay = 2.f * (qx * qy + qw * qz);
  const float cross = ay * wx - ax * wy;
  const bool up_left = cross > 0.f;

  const unsigned int key = p.seed ^ ((unsigned int)(p.first_world + w) * 0x9E3779B9u) ^ (tick * 0x85EBCA6Bu);
  const float u0 = nav_uniform(key, 8u), u1 = nav_uniform(key, 9u), u2 = nav_uniform(key, 10u);
  const float p_stop = nav_clamp(p.dt * (p.lambda_ws0 + p.dlambda_ws * k_stop), 0.f, 1.f);
  const float p_walk = nav_clamp(p.dt * (p.lambda_sw0 + p.dlambda_sw * k_walk), 0.f, 1.f);
  const float p_turn = nav_clamp(p.dt * p.lambda_turn, 0.f, 1.f);
  const float p_up = nav_clamp(p.p_up0 + p.up_gain * freq, p.p_up_min, p.p_up_max);

  int next = state, remaining = P.remaining[w];
  if (state == NMF_NAV_WALK) {
    if (u0 < p_stop) next = NMF_NAV_STOP;
    else if (u1 < p_turn) {
      const bool upwind = u2 < p_up;
      next = upwind == up_left ? NMF_NAV_TURN_LEFT : NMF_NAV_TURN_RIGHT;
      remaining = p.turn_ticks;
    }
  } else if (state == NMF_NAV_STOP) {
    if (u0 < p_walk) next = NMF_NAV_WALK;
  } else {
    remaining = (int)((unsigned int)remaining - 1u);
    if (remaining <= 0) next = NMF_NAV_WALK;
  }

  P.state[w] = next;
  P.remaining[w] = remaining;
  P.above[w] = now ? 1 : 0;
  P.k_stop[w] = k_stop;
  P.k_walk[w] = k_walk;
  P.freq[w] = freq;
  P.ticks[w] = tick + 1u;
  P.encounters[w] = (int)((unsigned int)P.encounters[w] + (e ? 1u : 0u));
  reinterpret_cast<float2*>(drive_out)[w] = nav_drive(p, next);
}

// WALK, no turn under way, not above the threshold, empty filters, tick 0, no encounters and the walk drive in the handle's own
// drive array, for the worlds of the mask (all when mask is null); one lane per world
__global__ void nmf_navigator_reset_kernel(NavArgs A, NavPtrs P, const uint8_t* __restrict__ mask) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= A.n_worlds) return;
  if (mask && !mask[w]) return;
  P.state[w] = NMF_NAV_WALK;
  P.remaining[w] = 0;
  P.above[w] = 0;
  P.k_stop[w] = 0.f;
  P.k_walk[w] = 0.f;
  P.freq[w] = 0.f;
  P.ticks[w] = 0u;
  P.encounters[w] = 0;
  reinterpret_cast<float2*>(P.drive)[w] = nav_drive(A.p, NMF_NAV_WALK);
}

}  // namespace nmf
