// nmf_cpg.hip — closed-loop steerable tripod CPG on the device (gfx950): flygym_amd.controllers.TurningCPG.
//
// No reference counterpart (the snapshot has no CPG): build-defined; the specification in numpy is
// tests/cpg_spec.py.  Per world six coupled phase oscillators (legs in LEGS order lf lm lh rf rm rh: side = leg / 3, tripod bias
// b = pi * (leg & 1)) with phase theta (cycles, float64) and magnitude r (float32), and a drive d = (d_left, d_right).  One step,
// every right-hand side from the old state:
//
//   row       c = (1 - f) cycle[i0][col] + f cycle[i0 + 1][col],  x = theta n_bins, i0 = floor(x) mod n_bins, f = x - floor(x)
//             target[col] = c + (r - 1) (c - mean[col]);  adhesion[l] = stance[i0][l] ? on : off
//   theta_l <- (theta_l + dt (nu sign(d) + (1 / 2 pi) sum_{j != l} r_j w sin(2 pi (theta_j - theta_l) - (b_j - b_l)))) mod 1
//   r_l     <- r_l + dt a (|d| - r_l)
//
// The phase, its bin position x and its increment dt (nu + S / 2 pi) are float64 — a float32 phase drifts 4e-5 cycles in 2500
// steps, and dt nu rounded to float32 still 2e-7 —; the coupling sum S, the sines and the rows are float32.  The magnitude every
// formula reads is float32 too, but its Euler sum is kept in a float64 shadow beside the public float32 array: 400 float32
// additions wander up to 17 ulp from the float64 recurrence (measured on the specification), the shadow's rounding stays below
// one.  A magnitude the caller wrote (public value != the shadow's rounding) replaces the shadow at the next launch.
//
// One launch advances all worlds by n_steps and writes n_steps rows per world into the table nmf_step_replay reads.  A workgroup
// owns kCpgWorlds consecutive worlds and alternates, in passes of up to kCpgChunk steps:
//   phase A  the recurrence, sequential in the step: wave 0, one lane per (world, leg), ten worlds in 60 lanes; the other five
//            legs' (theta, r) come by ds_bpermute from lanes base + j, j = 0..5 in this order for every lane, so a world's sums
//            do not depend on where in a wave it sits (bitwise batch independence).  (bin, fraction, r) of every step go to LDS.
//   phase B  all lanes expand the pass's (world, step, column) items: the shared cycle table (n_bins x n_pos floats, 43 KB at
//            42 columns: L2 / L1 resident) is read from global memory, and the rows of a world — contiguous in the table — are
//            written as whole coalesced segments.
//
// The hybrid advance (flygym_amd.controllers.HybridTurningCPG; specification tests/hybrid_spec.py; build-defined like the CPG, in
// the form of flygym 1.x's hybrid controller, default constants as remembered from it) adds two sensory rules that lift a leg by
// adding net_l * corr[col] to its targets; the oscillators are not touched.  State per (world, leg): retraction rho and stumbling
// sigma, float32 in [0, cap].  The decision is taken once per launch from the batch's seg_xpos / seg_xquat / sensordata as they
// stand when the launch starts, and held for all its steps:
//   h_l = z(root segment) - z(tip segment of leg l); L* = the leg of the largest h (ties: the lowest index), h3 = the third largest
//   retract[L*] = h_L* > h3 + retraction_threshold                                   (at most one leg per world)
//   stumble[l]  = swing[i0_l][l] and found_l > 0 and F_l . xhat < -stumbling_force_threshold      (i0_l: the bin at launch start)
// with xhat the root segment's x axis in the world and F_l the leg's net sensor force in the world frame (rebuilt from the
// reported normal and tangent, third axis n x t1 as make_frame / contact_frame define it, where the model reports it in the
// contact frame).  Per step, from the state before its update:
//   net_l = rho_l > 0 ? rho_l : sigma_l;  target[col] = fl(cpg target + fl(net_l corr[col]));  adhesion[l] = off while net_l > 0
//   rho_l   <- retract[l] ? min(rho_l + up_r, cap)   : max(rho_l - down_r, 0)
//   sigma_l <- stumble[l] ? min(sigma_l + up_s, cap) : max(sigma_l - down_s, 0)
// Phase A's lanes read their world's six h by ds_bpermute like the coupling sum (the third largest by rank counting) and write
// net of every step to a fourth LDS array; phase B adds the correction with two separate roundings (no contraction).
#include "nmf_device.h"

namespace nmf {

constexpr int kCpgThreads = 256;
constexpr int kCpgWorlds = 10;               // worlds per workgroup: 60 of wave 0's lanes run the recurrence
constexpr int kCpgLanes = 6 * kCpgWorlds;
constexpr int kCpgChunk = 32;                // steps per pass: 3 (hybrid: 4) x 32 x 60 words of LDS

struct CpgArgs {
  int n_worlds, n_pos, n_act, n_bins;        // n_act = n_pos (+ 6 adhesion columns when the plan has stance bins)
  double frequency, timestep;
  float coupling, convergence, adhesion_on, adhesion_off;
};

struct CpgHybridArgs {
  int nseg, root_seg, contact_frame;         // contact_frame: the sensor reports its force in the contact frame
  int tip_seg[6];
  float retraction_threshold, stumbling_force_threshold, up_r, down_r, up_s, down_s, cap;
};

// the rules' state and the batch arrays the decision reads (all null for the plain advance)
struct CpgHybridPtrs {
  const float* corr; const uint8_t* swing;
  const float* seg_xpos; const float* seg_xquat; const float* sensordata;
  float* retraction; float* stumbling; uint8_t* flags;
};

// v + a b with the product and the sum rounded separately (the specification's two float32 roundings)
__device__ __forceinline__ float add_product(float v, float a, float b) {
#pragma clang fp contract(off) reassociate(off)
  const float p = a * b;
  return v + p;
}

// theta = (world / total + b / 2 pi) mod 1, r = 1, drive = (1, 1) for the worlds of the mask (all when mask is null)
__global__ void nmf_cpg_reset_kernel(int n_worlds, const uint8_t* __restrict__ mask, int first_world, int total_worlds,
                                     double* __restrict__ phase, float* __restrict__ mag, double* __restrict__ mag_acc,
                                     float* __restrict__ drive) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 6 * n_worlds) return;
  const int w = i / 6, leg = i - 6 * w;
  if (mask && !mask[w]) return;
  const double x = __ddiv_rn((double)(first_world + w), (double)total_worlds) + 0.5 * (double)(leg & 1);   // (no reciprocal: the host's w / n)
  phase[i] = x - floor(x);
  mag[i] = 1.f;
  mag_acc[i] = 1.0;
  if (leg < 2) drive[2 * w + leg] = 1.f;
}

// The body of both kernels.  The structs come by value and the pointers carry no __restrict__ of their own (the kernels' arguments
// do): with references or repeated qualifiers the plain instantiation's schedule drifts from the code it had as a kernel of its own.
template <bool HYBRID>
__device__ __forceinline__ void cpg_advance(const CpgArgs A, const float* cycle, const float* mean, const int* leg_of_col,
                                            const uint8_t* stance, const float* drive, double* phase, float* mag, double* mag_acc,
                                            float* table, int table_steps, int n_steps, const CpgHybridArgs H, const CpgHybridPtrs P) {
  __shared__ int s_bin[kCpgChunk][kCpgLanes];
  __shared__ float s_frac[kCpgChunk][kCpgLanes];
  __shared__ float s_mag[kCpgChunk][kCpgLanes];
  __shared__ float s_net[HYBRID ? kCpgChunk : 1][kCpgLanes];
  constexpr float kTwoPi = 6.28318530717958647692f, kPi = 3.14159265358979323846f;
  constexpr double kInvTwoPi = 0.15915494309189533577;
  const int tid = threadIdx.x;
  const int w0 = blockIdx.x * kCpgWorlds;
  const int nw = min(kCpgWorlds, A.n_worlds - w0);
  // wave 0: lane = 6 * (world in the group) + leg; the lanes past the group's worlds run along on zeros and store nothing
  const int leg = tid % 6, base = tid - leg;
  const bool osc = tid < 6 * nw;
  double th = 0.0, nu = 0.0, racc = 0.0, R = 0.0;
  if (osc) {
    const size_t k = (size_t)w0 * 6 + (size_t)tid;
    const float d = drive[(size_t)(w0 + tid / 6) * 2 + (size_t)(leg / 3)];
    th = phase[k];
    const float pub = mag[k];
    racc = mag_acc[k];
    if ((float)racc != pub) racc = (double)pub;
    R = (double)fabsf(d);
    nu = d > 0.f ? A.frequency : (d < 0.f ? -A.frequency : 0.0);
  }
  const double rate = A.timestep * (double)A.convergence;
  float rho = 0.f, sigma = 0.f;
  bool retract = false, stumble = false;
  if constexpr (HYBRID) {
    if (tid < kWave) {
      float h = 0.f, push = 0.f, found = 0.f;
      bool swinging = false;
      if (osc) {
        const size_t w = (size_t)(w0 + tid / 6), k = (size_t)w0 * 6 + (size_t)tid;
        rho = P.retraction[k];
        sigma = P.stumbling[k];
        const float* xp = P.seg_xpos + w * (size_t)H.nseg * 3;
        h = xp[3 * H.root_seg + 2] - xp[3 * H.tip_seg[leg] + 2];
        const float* q = P.seg_xquat + (w * (size_t)H.nseg + (size_t)H.root_seg) * 4;
        const float qw = q[0], qx = q[1], qy = q[2], qz = q[3];
        const float ax = 1.f - 2.f * (qy * qy + qz * qz), ay = 2.f * (qx * qy + qw * qz), az = 2.f * (qx * qz - qw * qy);
        const float* sd = P.sensordata + w * 96 + 16 * (size_t)leg;
        found = sd[0];
        float fx = sd[1], fy = sd[2], fz = sd[3];
        if (H.contact_frame) {                     // (normal, t1, t2) components: t2 = n x t1
          const float nx = sd[10], ny = sd[11], nz = sd[12], tx = sd[13], ty = sd[14], tz = sd[15];
          const float ux = ny * tz - nz * ty, uy = nz * tx - nx * tz, uz = nx * ty - ny * tx;
          const float fn = fx, f1 = fy, f2 = fz;
          fx = fn * nx + f1 * tx + f2 * ux; fy = fn * ny + f1 * ty + f2 * uy; fz = fn * nz + f1 * tz + f2 * uz;
        }
        push = fx * ax + fy * ay + fz * az;
        const double x0 = floor(th * (double)A.n_bins);   // (a NaN or huge phase the caller wrote must not index outside swing)
        const int bin = fabs(x0) < 2147483648.0 ? (int)x0 % A.n_bins : 0;
        swinging =P.swing[(size_t)(bin < 0 ? bin + A.n_bins : bin) * 6 + leg] != 0;
      }
      // the world's six h, from lanes base + j in the same order for every lane; rank = the legs that come before in the order
      // "larger h first, ties to the lower index": rank 0 is L*, rank 2 holds the third largest
      float hj[6];
#pragma unroll
      for (int j = 0; j < 6; ++j) hj[j] = __shfl(h, base + j);
      int mine = 0;
      float h3 = 0.f;
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        int rank = 0;
#pragma unroll
        for (int k = 0; k < 6; ++k) rank += (hj[k] > hj[j] || (hj[k] == hj[j] && k < j)) ? 1 : 0;
        if (rank == 2) h3 = hj[j];
        if (j == leg) mine = rank;
      }
      retract = osc && mine == 0 && h > h3 + H.retraction_threshold;
      stumble = osc && swinging && found > 0.f && push < -H.stumbling_force_threshold;
      if (osc) P.flags[(size_t)w0 * 6 + (size_t)tid] = (uint8_t)((retract ? 1 : 0) | (stumble ? 2 : 0));
    }
  }
  for (int s0 = 0; s0 < n_steps; s0 += kCpgChunk) {
    const int ns = min(kCpgChunk, n_steps - s0);
    if (tid < kWave) {
      for (int s = 0; s < ns; ++s) {
        const double x = th * (double)A.n_bins, fl = floor(x);
        const float r = (float)racc;
        if (osc) {
          const int bin = (int)fl % A.n_bins;       // (a phase the caller wrote outside [0, 1) must not index outside the cycle)
          s_bin[s][tid] = bin < 0 ? bin + A.n_bins : bin;
          s_frac[s][tid] = (float)(x - fl);
          s_mag[s][tid] = r;
        }
        if constexpr (HYBRID) {
          if (osc) s_net[s][tid] = rho > 0.f ? rho : sigma;
          rho = retract ? fminf(rho + H.up_r, H.cap) : fmaxf(rho - H.down_r, 0.f);
          sigma = stumble ? fminf(sigma + H.up_s, H.cap) : fmaxf(sigma - H.down_s, 0.f);
        }
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          const double thj = __shfl(th, base + j);
          const float rj = __shfl(r, base + j);
          const float arg = kTwoPi * (float)(thj - th) - kPi * (float)((j & 1) - (leg & 1));
          const float term = rj * A.coupling * sinf(arg);
          if (j != leg) sum += term;
        }
        th += A.timestep * (nu + (double)sum * kInvTwoPi);
        th -= floor(th);
        if (th >= 1.0) th = 0.0;                  // (-tiny mod 1 rounds to 1)
        racc += rate * (R - racc);
      }
    }
    __syncthreads();
    const int seg = ns * A.n_act, total = nw * seg;
    for (int i = tid; i < total; i += kCpgThreads) {
      const int wl = i / seg, rem = i - wl * seg;
      const int s = rem / A.n_act, col = rem - s * A.n_act;
      float v;
      if (col < A.n_pos) {
        const int lane = 6 * wl + leg_of_col[col];
        const int i0 = s_bin[s][lane], i1 = i0 + 1 == A.n_bins ? 0 : i0 + 1;
        const float f = s_frac[s][lane];
        const float c = (1.f - f) * cycle[(size_t)i0 * A.n_pos + col] + f * cycle[(size_t)i1 * A.n_pos + col];
        v = c + (s_mag[s][lane] - 1.f) * (c - mean[col]);
        if constexpr (HYBRID) v = add_product(v, s_net[s][lane], P.corr[col]);
      } else {
        const int l = col - A.n_pos;
        v = stance[(size_t)s_bin[s][6 * wl + l] * 6 + l] ? A.adhesion_on : A.adhesion_off;
        if constexpr (HYBRID) { if (s_net[s][6 * wl + l] > 0.f) v = A.adhesion_off; }
      }
      table[((size_t)(w0 + wl) * (size_t)table_steps + (size_t)s0) * (size_t)A.n_act + (size_t)rem] = v;
    }
    __syncthreads();
  }
  if (osc) {
    const size_t k = (size_t)w0 * 6 + (size_t)tid;
    phase[k] = th;
    mag[k] = (float)racc;
    mag_acc[k] = racc;
    if constexpr (HYBRID) { P.retraction[k] = rho; P.stumbling[k] = sigma; }
  }
}

__global__ void __launch_bounds__(kCpgThreads)
nmf_cpg_advance_kernel(CpgArgs A, const float* __restrict__ cycle, const float* __restrict__ mean, const int* __restrict__ leg_of_col,
                       const uint8_t* __restrict__ stance, const float* __restrict__ drive, double* __restrict__ phase,
                       float* __restrict__ mag, double* __restrict__ mag_acc, float* __restrict__ table, int table_steps, int n_steps) {
  cpg_advance<false>(A, cycle, mean, leg_of_col, stance, drive, phase, mag, mag_acc, table, table_steps, n_steps, CpgHybridArgs{},
                     CpgHybridPtrs{});
}

__global__ void __launch_bounds__(kCpgThreads)
nmf_cpg_advance_hybrid_kernel(CpgArgs A, CpgHybridArgs H, CpgHybridPtrs P, const float* __restrict__ cycle, const float* __restrict__ mean,
                              const int* __restrict__ leg_of_col, const uint8_t* __restrict__ stance, const float* __restrict__ drive,
                              double* __restrict__ phase, float* __restrict__ mag, double* __restrict__ mag_acc,
                              float* __restrict__ table, int table_steps, int n_steps) {
  cpg_advance<true>(A, cycle, mean, leg_of_col, stance, drive, phase, mag, mag_acc, table, table_steps, n_steps, H, P);
}

// rho = sigma = 0 and no flag for the worlds of the mask (all when mask is null)
__global__ void nmf_cpg_hybrid_reset_kernel(int n_worlds, const uint8_t* __restrict__ mask, float* __restrict__ retraction,
                                            float* __restrict__ stumbling, uint8_t* __restrict__ flags) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 6 * n_worlds) return;
  if (mask && !mask[i / 6]) return;
  retraction[i] = 0.f;
  stumbling[i] = 0.f;
  flags[i] = 0;
}

}  // namespace nmf
