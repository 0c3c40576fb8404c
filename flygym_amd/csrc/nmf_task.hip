// nmf_task.hip — the walking task on the device (gfx950): flygym_amd.tasks.WalkingTask.
//
// No reference counterpart (the snapshot holds no tasks): build-defined and pinned by nothing, in the form of the Gymnasium
// environments flygym 1.x put around a walking fly; the statement of the rule is include/nmf.h (nmf_task_update), its
// specification in numpy tests/task_spec.py.  One launch per control tick reads the root's pose and velocity, the chosen actuators'
// forces and joint velocities, the legs' contact sensors, the chosen joint angles and the handle's course and goal as they stand
// when it starts and, per world, decides reward, termination and truncation, keeps the episode's accounts, starts the next
// episode where one ended, and writes the observation row.
//
// Layout: a group of 16 lanes per world — a DPP row —, four worlds per wave, 16 per workgroup of 256 lanes (256 workgroups at 4096
// worlds).  A world's row is about 2 x 42 forces and velocities, 42 angles, 24 sensor floats and 60 floats written: with a lane
// per world every one of those accesses would be strided by a whole row of the batch; with a group per world lane j takes
// actuators j, j + 16, ..., leg j (j < 6) and observation entries j, j + 16, ..., so the observation row is written in runs of
// 64 contiguous bytes and the gathers of one world fall into the few cache lines of its rows.  The root's pose, the free
// joint's velocity and the per-world state are read by all 16 lanes from one address (one request per group) and the scalar
// rule is evaluated by all of them alike — a lane working alone would cost the same issue slots —, lane 0 of the group stores
// it.  The power sum is int32, reduced over the row by four DPP adds (quad permutes, half mirror, mirror: every lane ends with
// the total), so its bits do not depend on the layout; the `bad` flag and the six contact flags are two wave ballots, shifted
// to the group's 16 bits.  No LDS, no atomics, no division, no square root, no function call.  The groups past the last world
// compute the last world again and store nothing, so every lane of a wave is live at the ballots and the DPP adds.  All
// arithmetic is compiled without contraction and reassociation and every clamp is a pair of comparisons, so kernel and
// specification agree bit for bit; a stored zero is made +0 in integer arithmetic (nmf_exact.h: the library's -fno-signed-zeros).
// The one-lane-per-world layout was not built: the time of this one is in profiles/task_summary.md.
#include "nmf.h"
#include "nmf_device.h"
#include "nmf_exact.h"

namespace nmf {

constexpr int kTaskGroup = 16;                              // lanes per world
constexpr int kTaskThreads = 256;
constexpr int kTaskWorlds = kTaskThreads / kTaskGroup;      // worlds per workgroup

struct TaskArgs {
  nmf_task_params p;
  int n_worlds, nseg, nq, nv, nu, sens_stride, obs_width;
};

// the batch arrays an update reads, the handle's tables and the per-world arrays (in the order of the NMF_TASK_ field indices)
struct TaskPtrs {
  const float *seg_xpos, *seg_xquat, *qpos, *qvel, *actuator_force, *sensordata;
  const int *act, *act_dof, *obs_dof;
  const float *mean, *inv_std;
  float *reward, *obs, *ep_return, *last_return, *prev_xy, *course, *goal;
  uint8_t *terminated, *truncated, *done, *fresh;
  int *reason, *ep_length, *last_length, *last_reason, *tilt_count, *airborne_count, *episodes, *successes;
};

// all exponent bits set: NaN, +Inf, -Inf.  On the bits: the library's fast-math flags leave isfinite to the compiler
__device__ __forceinline__ unsigned int task_odd(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u ? 1u : 0u; }

// v summed over the 16 lanes of a row, in every lane of it
__device__ __forceinline__ int task_row_sum(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false);       // quad_perm [1, 0, 3, 2]
  v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, false);       // quad_perm [2, 3, 0, 1]
  v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, false);      // row_half_mirror
  v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, false);      // row_mirror
  return v;
}

__global__ void __launch_bounds__(kTaskThreads)
nmf_task_update_kernel(TaskArgs A, TaskPtrs P) {
#pragma clang fp contract(off) reassociate(off)
  const int j = (int)(threadIdx.x & (kTaskGroup - 1));
  const int shift = (int)(threadIdx.x & 48u);                // of the group's 16 bits in a wave ballot
  const int w = (int)blockIdx.x * kTaskWorlds + (int)(threadIdx.x / kTaskGroup);
  const bool live = w < A.n_worlds;
  const size_t row = (size_t)(live ? w : A.n_worlds - 1);
  const nmf_task_params& p = A.p;

  // what every lane of the group reads from one address
  const float* __restrict__ xp = P.seg_xpos + (row * (size_t)A.nseg + (size_t)p.root_seg) * 3;
  const float x = xp[0], y = xp[1], z = xp[2];
  const float4 q = *reinterpret_cast<const float4*>(P.seg_xquat + (row * (size_t)A.nseg + (size_t)p.root_seg) * 4);
  const float qw = q.x, qx = q.y, qy = q.z, qz = q.w;
  const float* __restrict__ qvel = P.qvel + row * (size_t)A.nv;
  const float vx = qvel[0], vy = qvel[1], vz = qvel[2], ox = qvel[3], oy = qvel[4], oz = qvel[5];
  const float2 c = reinterpret_cast<const float2*>(P.course)[row];
  const float2 g = reinterpret_cast<const float2*>(P.goal)[row];
  unsigned int odd = task_odd(x) | task_odd(y) | task_odd(z) | task_odd(qw) | task_odd(qx) | task_odd(qy) | task_odd(qz) | task_odd(vx) |
                     task_odd(vy) | task_odd(vz) | task_odd(ox) | task_odd(oy) | task_odd(oz) | task_odd(c.x) | task_odd(c.y) | task_odd(g.x) |
                     task_odd(g.y);

  // the lane's actuators: the integer power terms
  const float* __restrict__ force = P.actuator_force + row * (size_t)A.nu;
  int psum = 0;
  for (int a = j; a < p.n_act; a += kTaskGroup) {
    const float f = force[P.act[a]], qd = qvel[6 + P.act_dof[a]];
    const unsigned int o = task_odd(f) | task_odd(qd);
    odd |= o;
    const float m = __builtin_fabsf(f * qd);
    const float cl = m < 0.f ? 0.f : (m > p.power_clip ? p.power_clip : m);
    const float scaled = o ? 0.f : cl * (float)(1 << NMF_TASK_POWER_BITS);
    psum += (int)__builtin_rintf(scaled);
  }
  psum = task_row_sum(psum);

  // the lane's leg (lanes 0..5): found, Fx, Fy, Fz
  const int leg = j < 6 ? j : 0;
  const float4 s = *reinterpret_cast<const float4*>(P.sensordata + row * (size_t)A.sens_stride + 16 * leg);
  const float thr2 = leg == 0 ? p.thr2[0] : leg == 1 ? p.thr2[1] : leg == 2 ? p.thr2[2] : leg == 3 ? p.thr2[3] : leg == 4 ? p.thr2[4] : p.thr2[5];
  const float f2 = (s.y * s.y + s.z * s.z) + s.w * s.w;
  const bool touch = j < 6 && s.x > 0.f && f2 > thr2;
  odd |= task_odd(s.x) | task_odd(s.y) | task_odd(s.z) | task_odd(s.w);

  // the lane's joint angles: only whether they are finite; the observation loop below reads them again
  const float* __restrict__ ang = P.qpos + row * (size_t)A.nq + 7;
  for (int k = j; k < p.n_q; k += kTaskGroup) odd |= task_odd(ang[P.obs_dof[k]]);

  const bool bad = ((unsigned int)(__ballot(odd != 0u) >> shift) & 0xffffu) != 0u;
  const unsigned int flags = (unsigned int)(__ballot(touch) >> shift) & 0x3fu;

  // the rule: the same in every lane of the group
  const bool fresh = P.fresh[row] != 0;
  const float2 prev = reinterpret_cast<const float2*>(P.prev_xy)[row];
  const float progress = fresh ? 0.f : (x - prev.x) * c.x + (y - prev.y) * c.y;
  const float up_z = 1.f - 2.f * (qx * qx + qy * qy);
  const int tilt = up_z < p.cos_max_tilt ? (int)((unsigned int)P.tilt_count[row] + 1u) : 0;
  const int air = flags == 0u ? (int)((unsigned int)P.airborne_count[row] + 1u) : 0;
  const float power = (float)psum * (1.f / (float)(1 << NMF_TASK_POWER_BITS));
  const int n = (int)((unsigned int)P.ep_length[row] + 1u);
  const bool grace = n <= p.grace_ticks;
  const float dx = g.x - x, dy = g.y - y;
  int reason = 0;
  if (!grace && tilt >= p.tilt_ticks) reason |= NMF_TASK_TILTED;
  if (!grace && air >= p.airborne_ticks) reason |= NMF_TASK_AIRBORNE;
  if (!grace && (z < p.z_min || z > p.z_max)) reason |= NMF_TASK_HEIGHT;
  if (x < p.arena[0] || x > p.arena[1] || y < p.arena[2] || y > p.arena[3]) reason |= NMF_TASK_OUT_OF_ARENA;
  if (dx * dx + dy * dy < p.goal_radius2) reason |= NMF_TASK_GOAL;
  if (bad) reason = NMF_TASK_NONFINITE;
  const bool terminated = reason != 0;
  const bool truncated = !terminated && n >= p.max_ticks;
  const bool done = terminated || truncated;

  float r = p.alive;
  r = r + p.w_progress * progress;
  r = r - p.w_power * power;
  r = r - p.w_tilt * (1.f - up_z);
  if (reason & NMF_TASK_GOAL) r = r + p.bonus_goal;
  if (reason & ~NMF_TASK_GOAL) r = r - p.penalty_fail;
  if (bad) r = -p.penalty_fail;
  r = plus_zero(r);
  const float ret = plus_zero(P.ep_return[row] + r);

  // the observation row: the twelve body-level entries in every lane, entry i written by lane i mod 16
  const float r00 = 1.f - 2.f * (qy * qy + qz * qz), r01 = 2.f * (qx * qy - qw * qz), r02 = 2.f * (qx * qz + qw * qy);
  const float r10 = 2.f * (qx * qy + qw * qz), r11 = 1.f - 2.f * (qx * qx + qz * qz), r12 = 2.f * (qy * qz - qw * qx);
  const float r20 = 2.f * (qx * qz - qw * qy), r21 = 2.f * (qy * qz + qw * qx);
  const float body[NMF_TASK_OBS_BODY] = {-r20, -r21, -up_z,
                                         (r00 * vx + r10 * vy) + r20 * vz, (r01 * vx + r11 * vy) + r21 * vz, (r02 * vx + r12 * vy) + up_z * vz,
                                         ox, oy, oz, r00 * dx + r10 * dy, r01 * dx + r11 * dy, z};
  float* __restrict__ obs = P.obs + row * (size_t)A.obs_width;
  for (int i = j; i < A.obs_width; i += kTaskGroup) {
    float v;
    if (i < NMF_TASK_OBS_BODY) {
      v = body[0];
#pragma unroll
      for (int u = 1; u < NMF_TASK_OBS_BODY; ++u) v = i == u ? body[u] : v;
    } else if (i < NMF_TASK_OBS_BODY + 6) {
      v = (flags >> (i - NMF_TASK_OBS_BODY)) & 1u ? 1.f : 0.f;
    } else {
      const int k = i - (NMF_TASK_OBS_BODY + 6);
      v = (ang[P.obs_dof[k]] - P.mean[k]) * P.inv_std[k];
    }
    if (live) obs[i] = bad ? 0.f : plus_zero(v);
  }

  if (j != 0 || !live) return;
  P.reward[row] = r;
  P.terminated[row] = terminated ? 1 : 0;
  P.truncated[row] = truncated ? 1 : 0;
  P.done[row] = done ? 1 : 0;
  P.reason[row] = reason;
  if (done) {
    P.last_return[row] = ret;
    P.last_length[row] = n;
    P.last_reason[row] = reason;
    P.episodes[row] = (int)((unsigned int)P.episodes[row] + 1u);
    if (reason & NMF_TASK_GOAL) P.successes[row] = (int)((unsigned int)P.successes[row] + 1u);
  }
  P.ep_return[row] = done ? 0.f : ret;
  P.ep_length[row] = done ? 0 : n;
  P.tilt_count[row] = done ? 0 : tilt;
  P.airborne_count[row] = done ? 0 : air;
  P.fresh[row] = done ? 1 : 0;
  reinterpret_cast<float2*>(P.prev_xy)[row] = done ? make_float2(0.f, 0.f) : make_float2(x, y);
}

// every per-world array but course and goal zeroed and fresh = 1, for the worlds of the mask (all when mask is null); one lane per
// world
__global__ void nmf_task_reset_kernel(TaskArgs A, TaskPtrs P, const uint8_t* __restrict__ mask) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= A.n_worlds) return;
  if (mask && !mask[w]) return;
  P.reward[w] = 0.f; P.ep_return[w] = 0.f; P.last_return[w] = 0.f;
  reinterpret_cast<float2*>(P.prev_xy)[w] = make_float2(0.f, 0.f);
  P.terminated[w] = 0; P.truncated[w] = 0; P.done[w] = 0; P.fresh[w] = 1;
  P.reason[w] = 0; P.ep_length[w] = 0; P.last_length[w] = 0; P.last_reason[w] = 0;
  P.tilt_count[w] = 0; P.airborne_count[w] = 0; P.episodes[w] = 0; P.successes[w] = 0;
  float* obs = P.obs + (size_t)w * (size_t)A.obs_width;
  for (int i = 0; i < A.obs_width; ++i) obs[i] = 0.f;
}

}  // namespace nmf
