// nmf_rules.hip — rule-based walking on the device (gfx950): flygym_amd.controllers.RuleBasedController.
//
// No reference counterpart (the snapshot holds no controllers): build-defined and pinned by nothing, in the form of flygym 1.x's
// decentralised rule-based controller (Cruse's rules 1 to 3); the statement of the model is include/nmf.h
// (nmf_rules_advance), its specification in numpy tests/rules_spec.py.  Per (world, leg) an integer step counter k in [0, P), a
// stepping flag and a latched amplitude a; per world a drive (left, right) and a tick word.  A leg at k = 0 rests; a step runs the
// leg's cycle once, swing first, in P physics steps.  Per physics step the three rules score every leg from the six counters, the
// legs within the margin of the best positive score are eligible, and one of them, drawn by nmf_plume.hip's counter-based hash of
// (seed, global world index, tick, draw index NMF_RULES_DRAW), starts a step.
//
// One launch advances all worlds by n_steps and writes n_steps rows per world into the table nmf_step_replay reads: the two-phase
// shape of nmf_cpg.hip, for its reasons.  A workgroup owns kRulesWorlds consecutive worlds and alternates, in passes of up to
// kRulesChunk steps:
//   phase A  the recurrence, sequential in the step: wave 0, one lane per (world, leg), ten worlds in 60 lanes.  A lane derives
//            (swinging, p) from its own counter; the six pairs of its world come by __shfl from lanes base + j, j = 0..5 in this
//            order for every lane, the eligible set of a world is (ballot >> base) & 63 and the drawn leg is found in six
//            predicated steps: a world's result does not depend on where in a wave, workgroup or shard it sits.  (bin, fraction,
//            amplitude, lifted) of every step go to LDS.
//   phase B  all lanes expand the pass's (world, step, column) items from the shared cycle table into whole coalesced row segments.
// The counters, flags, amplitudes, scores and tick words live in device memory and are written back when the launch ends, so a
// captured launch continues, and draws fresh numbers, on every replay.  All arithmetic is compiled without contraction and
// reassociation and every clamp is a pair of comparisons: kernel and specification agree bit for bit.
#include "nmf.h"
#include "nmf_device.h"
#include "nmf_exact.h"

namespace nmf {

constexpr int kRulesThreads = 256;
constexpr int kRulesWorlds = 10;             // worlds per workgroup: 60 of wave 0's lanes run the recurrence
constexpr int kRulesLanes = 6 * kRulesWorlds;
constexpr int kRulesChunk = 32;              // steps per pass: 3 x 32 x 60 words + 32 x 60 bytes of LDS

struct RulesArgs {
  int n_worlds, n_pos, n_act, n_bins, period;  // n_act = n_pos (+ 6 adhesion columns)
  float margin, max_amplitude, adhesion_on, adhesion_off;
  unsigned int seed; int first_world;
};

// the shared tables and the per-world state
struct RulesPtrs {
  const float* cycle; const float* rest; const int* leg_of_col;       // rest[col] = cycle[start_bin[leg_of_col[col]]][col]
  const int* start_bin; const int* swing_steps; const float* weights; // [6], [6], [3][6][6] as [rule][src][tgt]
  int* counter; uint8_t* stepping; float* amplitude; float* drive; unsigned int* ticks; float* scores;
};

__global__ void __launch_bounds__(kRulesThreads)
nmf_rules_advance_kernel(RulesArgs A, RulesPtrs P, float* __restrict__ table, int table_steps, int n_steps) {
#pragma clang fp contract(off) reassociate(off)
  __shared__ int s_bin[kRulesChunk][kRulesLanes];
  __shared__ float s_frac[kRulesChunk][kRulesLanes];
  __shared__ float s_amp[kRulesChunk][kRulesLanes];
  __shared__ uint8_t s_lift[kRulesChunk][kRulesLanes];
  const int tid = threadIdx.x;
  const int w0 = blockIdx.x * kRulesWorlds;
  const int nw = min(kRulesWorlds, A.n_worlds - w0);
  // wave 0: lane = 6 * (world in the group) + leg; the lanes past the group's worlds run along on zeros and store nothing
  const int leg = tid % 6, base = tid - leg;
  const bool own = tid < 6 * nw;
  int k = 0, start = 0, swing = 1;
  bool stepping = false;
  float amp = 0.f, d = 0.f, score = 0.f;
  unsigned int tick = 0u, world_key = 0u;
  float w1[6] = {}, w2[6] = {}, w3[6] = {};
  if (own) {
    const size_t i = (size_t)w0 * 6 + (size_t)tid, w = (size_t)(w0 + tid / 6);
    k = P.counter[i] % A.period;             // (a counter the caller wrote outside [0, P) must not index outside the cycle)
    if (k < 0) k += A.period;
    stepping = P.stepping[i] != 0;
    amp = P.amplitude[i];
    d = P.drive[w * 2 + (size_t)(leg / 3)];
    tick = P.ticks[w];
    world_key = A.seed ^ ((unsigned int)(A.first_world + (int)w) * 0x9E3779B9u);
    start = P.start_bin[leg];
    swing = P.swing_steps[leg];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      w1[j] = P.weights[6 * j + leg];
      w2[j] = P.weights[36 + 6 * j + leg];
      w3[j] = P.weights[72 + 6 * j + leg];
    }
  }
  const bool driven = own && d != 0.f;
  const float latch = fabsf(d) > A.max_amplitude ? A.max_amplitude : fabsf(d);
  const float stance_steps = (float)(A.period - swing);
  unsigned int driven6 = 0u;                 // the world's legs whose side has a drive: the fallback's eligible set
  if (tid < kWave) driven6 = (unsigned int)(__ballot(driven) >> base) & 63u;
  for (int s0 = 0; s0 < n_steps; s0 += kRulesChunk) {
    const int ns = min(kRulesChunk, n_steps - s0);
    if (tid < kWave) {
      for (int s = 0; s < ns; ++s) {
        // the row, from the state before the update
        const bool swinging = k > 0 && k < swing;
        const double x = div_rn((double)(k * A.n_bins), (double)A.period), fl = floor(x);
        if (own) {
          const int bin = start + (int)fl;     // (k < P: floor(x) < n_bins)
          s_bin[s][tid] = bin >= A.n_bins ? bin - A.n_bins : bin;
          s_frac[s][tid] = (float)(x - fl);
          s_amp[s][tid] = amp;
          s_lift[s][tid] = swinging ? 1 : 0;
        }
        // the scores: the world's six (swinging, p) from lanes base + j, in the same order for every lane
        const int past = k - swing;
        const float p = past > 0 ? (float)div_rn((double)(float)past, (double)stance_steps) : 0.f;   // (float32 / float32, correctly rounded)
        float r1 = 0.f, r2 = 0.f, r3 = 0.f;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          const int sj = __shfl(swinging ? 1 : 0, base + j);
          const float pj = __shfl(p, base + j);
          if (sj) r1 += w1[j];
          if (pj > 0.f) {
            r2 += w2[j] * (1.f - pj);
            r3 += w3[j] * pj;
          }
        }
        score = plus_zero((r1 + r2) + r3);
        float best = 0.f;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          const float cj = __shfl(score, base + j);
          best = j == 0 || cj > best ? cj : best;
        }
        const float below = best - fabsf(best) * A.margin;
        const float threshold = below > 0.f ? below : 0.f;
        const bool eligible = driven && score >= threshold && score > 0.f && !stepping;
        const unsigned int stepping6 = (unsigned int)(__ballot(stepping) >> base) & 63u;
        unsigned int eligible6 = (unsigned int)(__ballot(eligible) >> base) & 63u;
        if (stepping6 == 0u && eligible6 == 0u) eligible6 = driven6;          // the fallback: the walk starts, or starts again
        // the draw: the j-th eligible leg in ascending order
        const unsigned int n = (unsigned int)__popc(eligible6);
        const unsigned int u = plume_hash(world_key ^ (tick * 0x85EBCA6Bu) ^ ((unsigned int)NMF_RULES_DRAW * 0xC2B2AE35u));
        const int pick = (int)__umulhi(u, n);
        int chosen = -1, seen = 0;
#pragma unroll
        for (int b = 0; b < 6; ++b) {
          const int set = (int)((eligible6 >> b) & 1u);
          if (set && seen == pick) chosen = b;
          seen += set;
        }
        if (leg == chosen) { stepping = true; amp = latch; }
        if (stepping) {
          ++k;
          if (k == A.period) { k = 0; stepping = false; }
        }
        ++tick;
      }
    }
    __syncthreads();
    const int seg = ns * A.n_act, total = nw * seg;
    for (int i = tid; i < total; i += kRulesThreads) {
      const int wl = i / seg, rem = i - wl * seg;
      const int s = rem / A.n_act, col = rem - s * A.n_act;
      float v;
      if (col < A.n_pos) {
        const int lane = 6 * wl + P.leg_of_col[col];
        const int i0 = s_bin[s][lane], i1 = i0 + 1 == A.n_bins ? 0 : i0 + 1;
        const float f = s_frac[s][lane];
        const float c = (1.f - f) * P.cycle[(size_t)i0 * A.n_pos + col] + f * P.cycle[(size_t)i1 * A.n_pos + col];
        const float rest = P.rest[col];
        v = rest + s_amp[s][lane] * (c - rest);
      } else {
        v = s_lift[s][6 * wl + (col - A.n_pos)] ? A.adhesion_off : A.adhesion_on;
      }
      table[((size_t)(w0 + wl) * (size_t)table_steps + (size_t)s0) * (size_t)A.n_act + (size_t)rem] = v;
    }
    __syncthreads();
  }
  if (own) {
    const size_t i = (size_t)w0 * 6 + (size_t)tid;
    P.counter[i] = k;
    P.stepping[i] = stepping ? 1 : 0;
    P.amplitude[i] = amp;
    P.scores[i] = score;
    if (leg == 0) P.ticks[(size_t)(w0 + tid / 6)] = tick;
  }
}

// k = 0, not stepping, a = 1, scores = 0, drive = (1, 1), tick 0 for the worlds of the mask (all when mask is null)
__global__ void nmf_rules_reset_kernel(int n_worlds, const uint8_t* __restrict__ mask, RulesPtrs P) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 6 * n_worlds) return;
  const int w = i / 6, leg = i - 6 * w;
  if (mask && !mask[w]) return;
  P.counter[i] = 0;
  P.stepping[i] = 0;
  P.amplitude[i] = 1.f;
  P.scores[i] = 0.f;
  if (leg < 2) P.drive[2 * w + leg] = 1.f;
  if (leg == 2) P.ticks[w] = 0u;
}

}  // namespace nmf
