// nmf_step_diag.h — diagnostic instrumentation of the stepping kernel: the per-stage cycle clocks (STAGE*, SUB*:
// -DNMF_STAGE_PROFILE) and the schedule trace (TRACE_*: -DNMF_SCHED_TRACE).  Both go into separate diagnostic libraries; in the
// product build every macro here expands to nothing.  Touches no LDS of the step: the stage clocks keep their own __shared__
// accumulators.
//
// Not self-contained: one of the stage headers that nmf_step.hip includes in stage order to form the stepping kernel's
// translation unit, and it relies on the ones before it.
#pragma once
#include "nmf_device.h"

namespace nmf {

// Optional per-stage cycle accounting (s_memtime deltas of wave 0 / lane 0), built only with
// -DNMF_STAGE_PROFILE into a separate diagnostic library; the product build has no trace of it.
#ifdef NMF_STAGE_PROFILE
#define NMF_NSTAGE 48
__device__ unsigned long long g_stage_cycles[NMF_NSTAGE];
struct StageClock { unsigned long long last; unsigned long long* acc; };
#define STAGE_INIT() __shared__ unsigned long long stage_acc_[NMF_NSTAGE]; StageClock sc_; sc_.acc = stage_acc_; \
  if (threadIdx.x < NMF_NSTAGE) stage_acc_[threadIdx.x] = 0; __syncthreads(); sc_.last = clock64()
#define STAGE_FLUSH() do { __syncthreads(); if (blockIdx.x == 0 && threadIdx.x < NMF_NSTAGE) g_stage_cycles[threadIdx.x] += stage_acc_[threadIdx.x]; } while (0)
#define STAGE_ARG , StageClock& sc_
#define STAGE_PASS , sc_
#define STAGE(k) do { if (threadIdx.x == 0) { unsigned long long t_ = clock64(); sc_.acc[k] += t_ - sc_.last; sc_.last = clock64(); } } while (0)
// sub-stages inside a non-inlined function (block 0 only, straight to the global accumulators 18..27)
#define SUB_T0() unsigned long long sub_t_ = clock64()
#define SUB_RESET() sub_t_ = clock64()
#define SUB(k) do { if (blockIdx.x == 0 && threadIdx.x == 0) { unsigned long long t_ = clock64(); g_stage_cycles[k] += t_ - sub_t_; sub_t_ = clock64(); } } while (0)
#define SUB_COUNT(k, n) do { if (blockIdx.x == 0 && threadIdx.x == 0) g_stage_cycles[k] += (unsigned long long)(n); } while (0)
#define SUBH_T0() unsigned long long subh_t_ = clock64()
#define SUBH(k) do { if (blockIdx.x == 0 && threadIdx.x == 0) { unsigned long long t_ = clock64(); g_stage_cycles[k] += t_ - subh_t_; subh_t_ = clock64(); } } while (0)
// (contact-space solve, every workgroup) eliminations beyond a step's first: [pivots of the elimination][leading pivots, in row
// order, that it shares with the elimination before it]; row 65: [0] = first eliminations (= solves).  scripts/resume_prefix.py
#define NMF_RESUME_ROWS 66
__device__ unsigned long long g_resume_hist[NMF_RESUME_ROWS][65];
#define RESUME_HIST(n, k) do { if (threadIdx.x == 0) atomicAdd(&g_resume_hist[n][k], 1ull); } while (0)
#else
#define RESUME_HIST(n, k)
#define SUBH_T0()
#define SUBH(k)
#define SUB_T0()
#define SUB_RESET()
#define SUB(k)
#define SUB_COUNT(k, n)
#define STAGE_INIT()
#define STAGE_ARG
#define STAGE_PASS
#define STAGE(k)
#define STAGE_FLUSH()
#endif

// Optional schedule trace (-DNMF_SCHED_TRACE, diagnostic library only): per workgroup of the last stepping launch — start and
// exit time (s_memrealtime, 100 MHz), items taken, shader cycles spent stepping / between items (ticket, state in, state out)
#ifdef NMF_SCHED_TRACE
__device__ unsigned long long g_sched_trace[4096][8];
#define TRACE_DECL() unsigned long long tr_busy_ = 0, tr_gap_ = 0, tr_items_ = 0, tr_mark_ = __builtin_amdgcn_s_memtime(), tr_sub_[3] = {0, 0, 0}, tr_sm_ = tr_mark_; const unsigned long long tr_t0_ = __builtin_amdgcn_s_memrealtime()
// sub-marks inside the gap between two items: 0 = state out issued, 1 = ticket known, 2 = world known (order looked up); the rest is the state load
#define TRACE_SUB(k) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); tr_sub_[k] += t_ - tr_sm_; tr_sm_ = t_; } while (0)
#define TRACE_SUB_RESET() do { tr_sm_ = __builtin_amdgcn_s_memtime(); } while (0)
#define TRACE_GAP_END() do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); tr_gap_ += t_ - tr_mark_; tr_mark_ = t_; } while (0)
#define TRACE_BUSY_END() do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); tr_busy_ += t_ - tr_mark_; tr_mark_ = t_; tr_items_++; } while (0)
#define TRACE_FLUSH() do { if (threadIdx.x == 0 && blockIdx.x < 4096) { unsigned long long* q_ = g_sched_trace[blockIdx.x]; TRACE_GAP_END(); q_[0] = tr_t0_; q_[1] = __builtin_amdgcn_s_memrealtime(); q_[2] = tr_items_; q_[3] = tr_busy_; q_[4] = tr_gap_; q_[5] = tr_sub_[0]; q_[6] = tr_sub_[1]; q_[7] = tr_sub_[2]; } } while (0)
#else
#define TRACE_SUB(k)
#define TRACE_SUB_RESET()
#define TRACE_DECL()
#define TRACE_GAP_END()
#define TRACE_BUSY_END()
#define TRACE_FLUSH()
#endif

}  // namespace nmf
