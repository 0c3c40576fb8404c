// nmf_batch_ops.hip — the batch's utility kernels that have nothing to do with stepping: indexed gather / scatter,
// observation packing for the multi-GPU exchange, and the world order of the next stepping launch.
#include "nmf_device.h"

namespace nmf {

// Indexed gather / scatter in caller order (replaces the reference's Warp kernels,
// src/flygym/warp/utils.py:29-127).
__global__ void nmf_gather_kernel(const float* __restrict__ src, int width, const int* __restrict__ ids,
                                  int n_ids, int group, float* __restrict__ dst, int n_worlds) {
  int per = n_ids * group;
  size_t total = (size_t)n_worlds * per;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    int w = (int)(i / per), k = (int)(i % per);
    dst[i] = src[(size_t)w * width + (size_t)ids[k / group] * group + (k % group)];
  }
}
__global__ void nmf_scatter_kernel(float* __restrict__ dstf, int width, const int* __restrict__ ids, int n_ids,
                                   const float* __restrict__ src, int n_worlds) {
  size_t total = (size_t)n_worlds * n_ids;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    int w = (int)(i / n_ids), k = (int)(i % n_ids);
    dstf[(size_t)w * width + ids[k]] = src[i];
  }
}

// The observation block of the multi-GPU exchange in one launch: per world [joint angles nj | joint velocities nj |
// position-actuator forces n_act | contact sensors 96] (what the reference reads with four getter kernels,
// warp/simulation.py:73-211), rows `stride` floats apart.
__global__ void nmf_pack_obs_kernel(const float* __restrict__ qpos, const float* __restrict__ qvel, const float* __restrict__ force,
                                    const float* __restrict__ sens, int nq, int nv, int nu, int nj, int n_act, int n_worlds,
                                    float* __restrict__ out, int stride) {
  const int width = 2 * nj + n_act + 96;
  const size_t total = (size_t)n_worlds * width;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int w = (int)(i / width), k = (int)(i % width);
    float v;
    if (k < nj) v = qpos[(size_t)w * nq + 7 + k];
    else if (k < 2 * nj) v = qvel[(size_t)w * nv + 6 + (k - nj)];
    else if (k < 2 * nj + n_act) v = force[(size_t)w * nu + (k - 2 * nj)];
    else v = sens[(size_t)w * 96 + (k - 2 * nj - n_act)];
    out[(size_t)w * stride + k] = v;
  }
}

// Block order for the next launch.  A launch of n_worlds > resident waves runs in rounds and lasts until its last wave
// finishes; a fly's cost (shader cycles of its last launch) follows its contacts and Newton iterations and spreads 2x
// over a gait cycle.  Measured on 4096 worlds (ms per 50-step launch: in-order / costliest first / other packings):
//   tripod CPG, phase offset 2 pi w / N (cost varies smoothly with w):  6.12 / 6.46 / 6.6-6.8
//   kinematic replay, clip partition w % 20 (neighbours unrelated):     6.94 / 6.07 / 6.2-6.4
// Neither order wins everywhere (waves that share a SIMD slow each other down, so costs do not add), hence the policy
// is measured, not modelled: every launch records its duration (first block start to last block end, s_memrealtime),
// a smoothed duration per step is kept for both orders (restarted when the launch length changes), the better one is
// used and the other re-tried every 32nd launch.  Costliest-first = one workgroup: min / max, 256-bin histogram of the quantised cost, exclusive prefix from
// the top bin, scatter.  Worlds are independent: the order changes the schedule only, never a result.
// force_policy >= 0 (NMF_ORDER = inorder / costliest, diagnostics) bypasses the measured choice and its bookkeeping.
__global__ void __launch_bounds__(1024) nmf_order_kernel(const float* __restrict__ cost, int n, int* __restrict__ order,
                                                         SchedState* __restrict__ sched, int n_steps, int force_policy) {
  __shared__ unsigned int lo, hi, hist[256], base[256];   // lo / hi: bit patterns of non-negative floats order like the floats
  __shared__ int policy;
  if (threadIdx.x == 0 && force_policy >= 0) { lo = 0xffffffffu; hi = 0u; policy = force_policy; }
  if (threadIdx.x == 0 && force_policy < 0) {
    lo = 0xffffffffu; hi = 0u;
    SchedState s = *sched;
    if (s.launches > 0 && s.t_last > s.t_first && s.last_steps > 0) {
      const float dur = (float)(s.t_last - s.t_first) / (float)s.last_steps;
      float& e = s.ema[s.last_policy];
      e = e == 0.f ? dur : 0.5f * e + 0.5f * dur;
    }
    if (n_steps != s.last_steps) { s.launches = 0; s.ema[0] = 0.f; s.ema[1] = 0.f; }   // a different launch shape: start over
    int p;
    if (s.launches < 2) p = s.launches;                                  // one launch each to seed the averages
    else {
      const int best = s.ema[1] < s.ema[0] ? 1 : 0;
      p = (s.launches & 31) == 31 ? 1 - best : best;
    }
    s.t_first = ~0ull; s.t_last = 0ull; s.last_policy = p; s.launches += 1; s.last_steps = n_steps;
    *sched = s;
    policy = p;
  }
  if (threadIdx.x < 256) hist[threadIdx.x] = 0u;
  __syncthreads();
  if (policy == 0) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) order[i] = i;
    return;
  }
  unsigned int mn = 0xffffffffu, mx = 0u;
  for (int i = threadIdx.x; i < n; i += blockDim.x) { const unsigned int c = __float_as_uint(cost[i]); mn = min(mn, c); mx = max(mx, c); }
  atomicMin(&lo, mn); atomicMax(&hi, mx);
  __syncthreads();
  const float l = __uint_as_float(lo); const float scale = 255.0f / fmaxf(__uint_as_float(hi) - l, 1.0f);
  for (int i = threadIdx.x; i < n; i += blockDim.x) atomicAdd(&hist[(int)((cost[i] - l) * scale)], 1u);
  __syncthreads();
  // exclusive prefix from the top bin: base[b] = sum of hist over bins above b (a wave-parallel scan, 8 doubling steps —
  // the serial loop over 256 bins was half of this kernel's 9 us)
  if (threadIdx.x < 256) base[threadIdx.x] = hist[255 - threadIdx.x];        // reversed: inclusive scan from the top
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    unsigned int v = 0u;
    if (threadIdx.x < 256 && (int)threadIdx.x >= off) v = base[threadIdx.x - off];
    __syncthreads();
    if (threadIdx.x < 256) base[threadIdx.x] += v;
    __syncthreads();
  }
  unsigned int excl = 0u;
  if (threadIdx.x < 256) excl = base[255 - threadIdx.x] - hist[threadIdx.x];   // bins above threadIdx.x
  __syncthreads();
  if (threadIdx.x < 256) base[threadIdx.x] = excl;
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += blockDim.x) order[atomicAdd(&base[(int)((cost[i] - l) * scale)], 1u)] = i;
}

}  // namespace nmf
