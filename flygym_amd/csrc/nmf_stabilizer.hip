// nmf_stabilizer.hip — head stabilization on the device (gfx950): flygym_amd.controllers.HeadStabilizer.
//
// No reference counterpart (the snapshot holds no controllers): build-defined and pinned by nothing, in the form of flygym 1.x's
// head-stabilization model — a small MLP from the leg joint angles and the leg contact flags to the neck's roll and pitch —
// DESIGN.md §7; the statement of the model is include/nmf.h (nmf_stabilizer_update), its specification in numpy
// tests/stabilizer_spec.py.  One stateless launch per control tick reads the batch's qpos and sensordata as they stand when it
// starts and, per world, standardises the chosen joint angles, thresholds the six legs' contact forces, evaluates up to four dense
// layers (ReLU between them), clamps the outputs and writes them to `out` and, when the handle has actuator ids, into ctrl.
//
// A workgroup is 64 worlds — a lane per world — times kStabWaves waves that share them (64 workgroups at 4096 worlds: a
// latency-bound launch, spread over as many CUs).  The inputs and the hidden activations live in LDS laid out [unit][lane]: every
// access is 64 consecutive words, free of bank conflicts.  Two buffers alternate between the layers, a workgroup barrier after
// each.  The weights are the same for every lane: the host uploads each layer transposed and padded, bias[jpad] then Wt[k][jpad]
// with jpad the layer's width rounded up to 8 (zero weights and biases in the padding), so that the eight weights of a block of
// outputs at one input are 32 contiguous, 32-byte aligned bytes behind a wave-uniform address: scalar loads, and the
// multiply-add takes its weight from a scalar register.  A lane holds a block of eight accumulators, so an activation is read
// from LDS once per block, not once per output; the blocks of a layer go round the waves (wave v takes blocks v, v +
// kStabWaves, ...), as do the inputs' units.  Every output's chain is a[j] = b[j], then a[j] = fmaf(W[j][k], h[k], a[j]) for
// ascending k, whole inside one lane — one rounding per multiply-add, the specification's order, whatever the split.  The rest
// is compiled without contraction and reassociation and every clamp is a pair of comparisons.  No division, no function call,
// no atomics, no state.  The lanes past the last world compute the last world again and store nothing.
#include "nmf.h"
#include "nmf_device.h"

namespace nmf {

constexpr int kStabLanes = 64;       // worlds per workgroup
constexpr int kStabWaves = 4;        // waves that share them
constexpr int kStabBlock = 8;        // accumulators per lane = the padding of a layer's width
constexpr int kStabMaxLayers = 4;    // three hidden layers and the output layer

struct StabArgs {
  int n_worlds, qpos_stride, sens_stride, ctrl_stride;
  int n_q, n_in, contacts, n_layers, drive;
  int width[kStabMaxLayers];         // outputs of layer i; width[n_layers - 1] = n_out
  int offset[kStabMaxLayers];        // of layer i in the weight blob, in floats: bias[jpad], then Wt[k][jpad]
  int lds_b;                         // first unit of the second LDS buffer
  int act[NMF_STABILIZER_MAX_OUT];
  float thr2[6], lo[NMF_STABILIZER_MAX_OUT], hi[NMF_STABILIZER_MAX_OUT];
};

// acc[u] = bias[j0 + u], then acc[u] = fmaf(Wt[k][j0 + u], h[k], acc[u]) for k = 0 .. n_prev - 1; h[k] is this lane's entry of
// LDS unit k of `in`
__device__ __forceinline__ void stab_block(float (&acc)[kStabBlock], const float* __restrict__ layer, int jpad, int j0, int n_prev,
                                           const float* in) {
#pragma clang fp contract(off) reassociate(off)
  const float* __restrict__ col = layer + jpad + j0;
#pragma unroll
  for (int u = 0; u < kStabBlock; ++u) acc[u] = layer[j0 + u];
#pragma unroll 8
  for (int k = 0; k < n_prev; ++k) {
    const float h = in[k * kStabLanes];
#pragma unroll
    for (int u = 0; u < kStabBlock; ++u) acc[u] = __builtin_fmaf(col[(size_t)k * (size_t)jpad + u], h, acc[u]);
  }
}

__global__ void __launch_bounds__(kStabLanes * kStabWaves)
nmf_stabilizer_update_kernel(StabArgs A, const float* __restrict__ qpos, const float* __restrict__ sensordata, const int* __restrict__ dof,
                             const float* __restrict__ mean, const float* __restrict__ inv_std, const float* __restrict__ blob,
                             float* __restrict__ ctrl, float* __restrict__ out) {
#pragma clang fp contract(off) reassociate(off)
  extern __shared__ float stab_lds[];
  const int lane = threadIdx.x & (kStabLanes - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kStabLanes));      // (a scalar: what it indexes stays wave-uniform)
  const int w = blockIdx.x * kStabLanes + lane;
  const bool live = w < A.n_worlds;
  const size_t row = (size_t)(live ? w : A.n_worlds - 1);
  float* const buf_a = stab_lds + lane;
  float* const buf_b = stab_lds + A.lds_b * kStabLanes + lane;

  // the inputs: standardised joint angles, then the six contact flags
  const float* __restrict__ q = qpos + row * (size_t)A.qpos_stride + 7;
  for (int k = wave; k < A.n_q; k += kStabWaves) buf_a[k * kStabLanes] = (q[dof[k]] - mean[k]) * inv_std[k];
  if (A.contacts) {
    const float4* __restrict__ s = reinterpret_cast<const float4*>(sensordata + row * (size_t)A.sens_stride);
    for (int l = wave; l < 6; l += kStabWaves) {
      const float4 f = s[4 * l];                                        // found, Fx, Fy, Fz
      const float m = __builtin_fmaf(f.w, f.w, __builtin_fmaf(f.z, f.z, f.y * f.y));
      buf_a[(A.n_q + l) * kStabLanes] = (f.x > 0.f && m > A.thr2[l]) ? 1.f : 0.f;
    }
  }
  __syncthreads();

  // the hidden layers: A -> B -> A -> B
  float* in = buf_a;
  float* to = buf_b;
  int n_prev = A.n_in;
  float acc[kStabBlock];
  for (int i = 0; i + 1 < A.n_layers; ++i) {
    const int width = A.width[i], jpad = (width + kStabBlock - 1) & ~(kStabBlock - 1);
    const float* __restrict__ layer = blob + A.offset[i];
    for (int j0 = wave * kStabBlock; j0 < width; j0 += kStabWaves * kStabBlock) {
      stab_block(acc, layer, jpad, j0, n_prev, in);
#pragma unroll
      for (int u = 0; u < kStabBlock; ++u)
        if (j0 + u < width) to[(j0 + u) * kStabLanes] = acc[u] > 0.f ? acc[u] : 0.f;
    }
    __syncthreads();
    float* t = in; in = to; to = t;
    n_prev = width;
  }

  // the output layer (one block: n_out <= 8, one wave), the clamp and the stores
  if (wave != 0 || !live) return;
  const int n_out = A.width[A.n_layers - 1];
  stab_block(acc, blob + A.offset[A.n_layers - 1], kStabBlock, 0, n_prev, in);
#pragma unroll
  for (int u = 0; u < kStabBlock; ++u) {
    if (u < n_out) {
      const float y = acc[u] < A.lo[u] ? A.lo[u] : (acc[u] > A.hi[u] ? A.hi[u] : acc[u]);
      out[row * (size_t)n_out + u] = y;
      if (A.drive) ctrl[row * (size_t)A.ctrl_stride + A.act[u]] = y;
    }
  }
}

}  // namespace nmf
