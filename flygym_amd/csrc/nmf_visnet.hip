// nmf_visnet.hip — a retinotopic visual network on the device (gfx950): flygym_amd.sensors.RetinotopicNetwork.
//
// No reference counterpart (the snapshot holds no vision processing): build-defined and pinned by nothing, in the form of the
// connectome-constrained networks of Lappalainen et al. 2024 that flygym 1.x's "advanced vision" task reads — cell types that are
// layers of one cell per ommatidium, joined by small convolution kernels on the hexagonal lattice and integrated as a leaky
// recurrent system — DESIGN.md §7; the statement of the model is include/nmf.h (nmf_visnet_update), its specification in numpy
// tests/visnet_spec.py.  Per (world, eye), `substeps` times with the same readings x0_i, x1_i:
//
//   r[c][i] = v[c][i] > 0 ? v[c][i] : +0                                       (of the OLD state of every type)
//   s = bias_c;  s = fmaf(in_w[c][0], x0_i, s);  s = fmaf(in_w[c][1], x1_i, s)
//   for the taps (pre, t, w) into c, in the caller's order:  j = neighbours[eye][t][i];  s = fmaf(w, j >= 0 ? r[pre][j] : +0, s)
//   d = s - v[c][i];  m = a_c d;  v[c][i] = v[c][i] + m
//
// then S[c] = sum_i (int) rint(min(r_new[c][i], 4) 2^16), pooled[c] = S[c] / (2^16 n_omm); and per world t = the fmaf chain of
// steer_w_c (pooled[left][c] - pooled[right][c]), the optomotor rule of nmf_motion.hip on gain t, and the drive.
//
// nmf_visnet_kernel: one workgroup per (world, eye), one thread per ommatidium (whole waves, up to 1024 threads).  A thread keeps
// the v[c] of its cell in registers over all sub-steps — a 32-element register vector that the loops over the types index with
// their wave-uniform c (relative register moves) — and the state is read from device memory once per update and written once.
// Dynamic LDS holds r as [type][n_omm + 1]: the last cell of every row stays +0 and is where a missing neighbour points, so a tap is one
// add and one ds_read_b32 with no select, and its fmaf executes like any other.  Beside it sits the neighbour table as uint16
// [T][n_omm] of the workgroup's eye (a missing neighbour stored as n_omm), copied from the handle's device copy once per
// workgroup, and the per-wave pooling partials.  At the limits that is 98,432 + 38,912 + 2,048 = 139,392 bytes of the CU's
// 163,840 (set with hipFuncSetAttribute at creation).  LDS is single-buffered: every new v is computed from the published r, barrier, the new r is
// published, barrier.  The per-type constants ride in the kernel arguments and the tap list (pre-row offset, table-row offset,
// weight: 16 bytes a tap, the same for every workgroup) is read behind wave-uniform addresses: scalar loads, and the multiply-add
// takes its weight from a scalar register.  Every chain is whole inside one lane in the specification's order; the rest is
// compiled without contraction and reassociation.  The pooling is an integer DPP reduction per wave (wave_reduce_bits) and the
// waves' partials are added from LDS in ascending order — integers: the order is immaterial.
//
// nmf_visnet_world_kernel: the second launch, a lane per world, from the pooled responses of its two eyes to signal and drive.
// The fresh bytes, one per (world, eye), live in device memory: a masked reset works and a captured update replays.  No atomics,
// no allocation; every pointer is a kernel argument or lives in the handle.
#include "nmf.h"
#include "nmf_device.h"
#include "nmf_exact.h"

namespace nmf {

constexpr int kVisMaxTypes = NMF_VISNET_MAX_TYPES;       // 32: the width of a cell's register vector
constexpr int kVisMaxThreads = 1024;
constexpr float kVisClamp = 4.f, kVisScale = 65536.f;    // a pooled term: clamped to 4, resolution 2^-16

struct VisArgs {
  nmf_visnet_params p;
  int n_worlds, n_omm, n_types, n_table, substeps;
  int row;                                     // n_omm + 1: cells of one type's LDS row, the last one +0
  int nb_word, part_word;                      // first 32-bit word of the neighbour table and of the partials in LDS
  int nb_words;                                // 32-bit words of the neighbour table (its uint16 count rounded up to even)
  double den;                                  // 2^16 n_omm, exact
  float bias[kVisMaxTypes], in_w0[kVisMaxTypes], in_w1[kVisMaxTypes], a[kVisMaxTypes], steer_w[kVisMaxTypes];
  int start[kVisMaxTypes + 1];                 // taps of type c: start[c] .. start[c + 1] - 1
};

// the per-world state and outputs of a handle (the shared tables are kernel arguments of their own: taps[n_taps] = (pre * row,
// t * n_omm, bits of w, 0) grouped by post type, and per eye the neighbour table as pairs of uint16, a missing neighbour = n_omm)
struct VisPtrs {
  float* v;                                    // [n_worlds][2][C][n_omm]
  uint8_t* fresh;                              // [n_worlds][2]
  int* sums;                                   // [n_worlds][2][C]
  float* pooled;                               // [n_worlds][2][C]
  float* signal;                               // [n_worlds]
};

__device__ __forceinline__ float vis_relu(float v) { return plus_zero(v > 0.f ? v : 0.f); }

// the cells of one ommatidium, one per type: a register vector, indexed by the wave-uniform type of the loops below
typedef float VisCells __attribute__((ext_vector_type(kVisMaxTypes)));

__global__ void __launch_bounds__(kVisMaxThreads)
nmf_visnet_kernel(VisArgs A, VisPtrs P, const int4* __restrict__ taps, const unsigned int* __restrict__ tables, const float2* __restrict__ omm) {
#pragma clang fp contract(off) reassociate(off)
  extern __shared__ float vis_lds[];
  const int i = (int)threadIdx.x, lane = i & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(i / kWave), n_waves = (int)blockDim.x / kWave;
  const int C = A.n_types, n_omm = A.n_omm, row = A.row;
  const bool cell = i < n_omm;
  const size_t eye = (size_t)blockIdx.x;                                   // world * 2 + eye
  float* const r = vis_lds;
  const unsigned short* const nb = reinterpret_cast<const unsigned short*>(vis_lds + A.nb_word);
  int* const part = reinterpret_cast<int*>(vis_lds + A.part_word);

  // the neighbour table of this eye, the zero cells, the state and the first r
  const unsigned int* __restrict__ table = tables + (size_t)(blockIdx.x & 1u) * (size_t)A.nb_words;
  for (int k = i; k < A.nb_words; k += (int)blockDim.x) reinterpret_cast<unsigned int*>(vis_lds + A.nb_word)[k] = table[k];
  if (i < C) r[i * row + n_omm] = 0.f;
  const bool fresh = P.fresh[eye] != 0;
  float* const state = P.v + eye * (size_t)C * (size_t)n_omm + (size_t)(cell ? i : 0);
  float x0 = 0.f, x1 = 0.f;
  if (cell) { const float2 x = omm[eye * (size_t)n_omm + (size_t)i]; x0 = x.x; x1 = x.y; }
  VisCells v = 0.f;
  if (cell) {
    for (int c = 0; c < C; ++c) {
      const float v0 = fresh ? A.bias[c] : state[(size_t)c * (size_t)n_omm];
      v[c] = v0;
      r[c * row + i] = vis_relu(v0);
    }
  }
  __syncthreads();

  for (int step = 0; step < A.substeps; ++step) {
    if (cell) {
      int k = 0;                                                           // (A.start[0])
      for (int c = 0; c < C; ++c) {
        float s = A.bias[c];
        s = __builtin_fmaf(A.in_w0[c], x0, s);
        s = __builtin_fmaf(A.in_w1[c], x1, s);
#pragma unroll 4
        for (const int k1 = A.start[c + 1]; k < k1; ++k) {
          const int4 tap = taps[k];
          const int j = (int)nb[tap.y + i];
          s = __builtin_fmaf(__int_as_float(tap.z), r[tap.x + j], s);
        }
        const float old = v[c];
        const float d = s - old;
        const float m = A.a[c] * d;
        v[c] = old + m;
      }
    }
    if (step + 1 < A.substeps) {                                           // (the last r is pooled from registers, not published)
      __syncthreads();
      if (cell)
        for (int c = 0; c < C; ++c) r[c * row + i] = vis_relu(v[c]);
      __syncthreads();
    }
  }

  // the state, and the pooled responses: a term per cell, an integer sum per wave, the waves' partials through LDS
  auto add = [](int a, int b) { return a + b; };
  for (int c = 0; c < C; ++c) {                                            // (wave-uniform: the ladder runs with every lane on)
    const float vc = v[c];
    int term = 0;
    if (cell) {
      state[(size_t)c * (size_t)n_omm] = vc;
      term = (int)rintf(fminf(vis_relu(vc), kVisClamp) * kVisScale);
    }
    term = wave_reduce_bits(term, 0, add);
    if (lane == 0) part[wave * kVisMaxTypes + c] = term;
  }
  __syncthreads();
  if (i < C) {
    int S = 0;
    for (int w = 0; w < n_waves; ++w) S += part[w * kVisMaxTypes + i];
    P.sums[eye * (size_t)C + (size_t)i] = S;
    P.pooled[eye * (size_t)C + (size_t)i] = (float)div_rn((double)S, A.den);
  }
  if (i == 0) P.fresh[eye] = 0;                                            // (every thread read it before the first barrier)
}

// signal and drive of one world from the pooled responses of its two eyes
__global__ void nmf_visnet_world_kernel(VisArgs A, VisPtrs P, const float* __restrict__ base, float* __restrict__ drive) {
#pragma clang fp contract(off) reassociate(off)
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= A.n_worlds) return;
  const nmf_visnet_params& p = A.p;
  const float* left = P.pooled + (size_t)w * 2 * (size_t)A.n_types;
  const float* right = left + A.n_types;
  float t = 0.f;
  for (int c = 0; c < A.n_types; ++c) {
    const float d = left[c] - right[c];
    t = __builtin_fmaf(A.steer_w[c], d, t);
  }
  t = plus_zero(t);
  const float g = p.gain * t;
  const float q = (float)div_rn((double)g, (double)(1.f + fabsf(g)));
  const float o[2] = {1.f - p.delta * fmaxf(q, 0.f), 1.f - p.delta * fmaxf(-q, 0.f)};
  P.signal[w] = t;
#pragma unroll
  for (int side = 0; side < 2; ++side) {
    const float b = base ? base[(size_t)w * 2 + side] : p.base;
    drive[(size_t)w * 2 + side] = fminf(fmaxf(b * o[side], p.drive_min), p.drive_max);
  }
}

// fresh = 1 for both eyes of the worlds of the mask (all when mask is null): their next update starts from v = bias
__global__ void nmf_visnet_reset_kernel(int n_worlds, const uint8_t* __restrict__ mask, uint8_t* __restrict__ fresh) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n_worlds) return;
  if (mask && !mask[w]) return;
  fresh[2 * w] = 1;
  fresh[2 * w + 1] = 1;
}

}  // namespace nmf
