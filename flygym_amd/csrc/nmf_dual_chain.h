// nmf_dual_chain.h — the elimination of the contact-space solve (nmf_dual.h): the chain of pivots, unrolled by ordinal, with the
// entries a step's later eliminations resume at.  Written over a per-lane number type F and six lane operations so that the
// same text is the device's code (F = float, the operations are the wave's instructions: the machine code is what it was when
// the chain stood in nmf_dual.h) and a host program's (F = ChainLanes, 64 plain floats: scripts/micro/dual_resume_check.cpp runs
// it under the address and undefined-behaviour sanitizers).  On the device it is one of the stage headers of the stepping
// kernel's translation unit and relies on the ones before it (readlane_f); on the host it stands alone.
#pragma once
#if !defined(__HIPCC__)
#include <cmath>
#endif

namespace nmf {

// the lane operations: the number lane kk holds (wave-uniform kk); a on lane kk, b elsewhere; a multiply-add per lane; 1 / sqrt
// of a wave-uniform number; the lowest row of a set (0 for an empty one); a scheduling barrier
#if defined(__HIPCC__)
#define NMF_CHAIN_FN __device__ __forceinline__
__device__ __forceinline__ float chain_readlane(float v, int kk) { return readlane_f(v, kk); }
__device__ __forceinline__ float chain_at_lane(int lane, int kk, float a, float b) { return lane == kk ? a : b; }
__device__ __forceinline__ float chain_fma(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ float chain_rsq(float d) { return __builtin_amdgcn_rsqf(d); }
__device__ __forceinline__ int chain_first(unsigned long long r) { return __builtin_amdgcn_readfirstlane(max(__ffsll((long long)r) - 1, 0)); }
__device__ __forceinline__ void chain_sched() { __builtin_amdgcn_sched_barrier(0); }
#else
#define NMF_CHAIN_FN inline
constexpr int kChainLanes = 64;
struct ChainLanes {       // a register of the wave as a plain array
  float v[kChainLanes];
  ChainLanes() { for (float& x : v) x = 0.f; }
  ChainLanes(float s) { for (float& x : v) x = s; }
  ChainLanes operator-() const { ChainLanes r; for (int i = 0; i < kChainLanes; ++i) r.v[i] = -v[i]; return r; }
  ChainLanes operator+(const ChainLanes& o) const { ChainLanes r; for (int i = 0; i < kChainLanes; ++i) r.v[i] = v[i] + o.v[i]; return r; }
  ChainLanes operator*(float s) const { ChainLanes r; for (int i = 0; i < kChainLanes; ++i) r.v[i] = v[i] * s; return r; }
};
inline float chain_readlane(const ChainLanes& x, int kk) { return x.v[kk]; }
inline ChainLanes chain_at_lane(int, int kk, const ChainLanes& a, const ChainLanes& b) { ChainLanes r = b; r.v[kk] = a.v[kk]; return r; }
inline ChainLanes chain_fma(const ChainLanes& a, float b, const ChainLanes& c) { ChainLanes r; for (int i = 0; i < kChainLanes; ++i) r.v[i] = std::fmaf(a.v[i], b, c.v[i]); return r; }
inline float chain_rsq(float d) { return 1.f / std::sqrt(d); }
inline int chain_first(unsigned long long r) { return r ? __builtin_ctzll(r) : 0; }
inline void chain_sched() {}
#endif

// Gauss-Jordan elimination of [R + A | b], left-looking, unrolled by pivot ORDINAL (the p-th active row, whatever its index):
// only the code of the pivots a step really has is ever fetched.  Lane i keeps cq[p] = (column of pivot p, row i) / sqrt(d_p),
// zero on the pivot's own row; the pivot row's entry at a later pivot column kk is that column's entry of row kk by symmetry
// of the not-yet-eliminated block — v_readlane(cq[q], kk) — so column kk of the current matrix is
//   A[.][kk] - sum_{q < p} cq[q] * cq[q](lane kk)      (two chains: the sum is a dependent sequence of multiply-adds).
// A's column kk is four reads of G (DualCol), requested a pivot ahead.  On return b holds the eliminated right-hand
// side, diag the pivot of the lane's own row — on this elimination's pivot rows only: on every other row it is unspecified (1, or when
// resuming whatever an earlier elimination of the step left there), so read it under the pivot mask.
// Resuming (KEEP > 0): cq[] and bsnap[] belong to the caller and outlive the call.  Everything ordinal p leaves behind depends on
// the first p pivots, G, R and the right-hand side only, so an elimination whose pivot set shares its first `start` pivots with
// the one these arrays come from enters the chain at ordinal `start` — a multiple of kDualSnap up to KEEP, 0 = from the top —
// with cq[0 .. start) as they are and b as it was there (bsnap: one copy every kDualSnap ordinals); diag keeps the pivots of the
// shared rows.  From `start` on it is the same instructions on the same numbers: not a bit changes.
constexpr int kDualSnap = 4;
// the ordinal an elimination of pivot set `mask` resumes at when the kept state comes from pivot set `mask_kept`: the pivots
// below the first row the two sets differ in, rounded down to an entry
template <int KEEP>
NMF_CHAIN_FN int dual_resume_ordinal(unsigned long long mask, unsigned long long mask_kept) {
  const unsigned long long df = mask ^ mask_kept;
  const int shared = __builtin_popcountll(mask & (df ? (df & (0ull - df)) - 1ull : ~0ull));
  const int entry = shared & -kDualSnap;
  return entry < KEEP ? entry : KEEP;
}
template <int PMAX, int KEEP, class F, class COL>
NMF_CHAIN_FN void dual_eliminate(unsigned long long rem, const COL& dc, F R, int lane, F& b, F& diag, F (&cq)[PMAX],
                                 F (&bsnap)[KEEP / kDualSnap + 1], int start) {
  static_assert(KEEP % kDualSnap == 0 && KEEP <= 16 && KEEP < PMAX, "entries of the ordinal chain: 4, 8, 12, 16");
  auto first_of = [](unsigned long long r) { return chain_first(r); };      // (0 for an empty set: a harmless fetch)
  if constexpr (KEEP > 0) { for (int i = 0; i < start; ++i) rem &= rem - 1ull; }      // (scalar: the shared pivots are done)
  int kk_next = first_of(rem);
  typename COL::Raw an = dc.fetch(kk_next);
  // (Round 6, measured and dropped: the two rows of a pyramid pair read the same four entries of G and differ in the sign of mu
  // only — skipping the reads and their address arithmetic when the next pivot is this one's pair mate costs a scalar branch per
  // pivot in front of the reads that are meant to be in flight early: 59.9 -> 59.0 M.)
#define NMF_DUAL_PIVOT(P)                                                                                   \
  if constexpr (P < PMAX) {                                                                                 \
    if (rem == 0ull) return;                                                                                \
    const int kk = kk_next;                                                                                 \
    rem &= rem - 1ull;                                                                                      \
    F col = dc.value(an) + chain_at_lane(lane, kk, R, 0.f);                                                         \
    kk_next = first_of(rem);                                                                                \
    an = dc.fetch(kk_next);                                                                                 \
    chain_sched();                          /* the next column's reads are in flight while this pivot's chain runs */ \
    { F c1 = 0.f;                                                                                           \
      _Pragma("unroll") for (int q = 0; q + 1 < P; q += 2) {                                                \
        col = chain_fma(-cq[q], chain_readlane(cq[q], kk), col); c1 = chain_fma(-cq[q + 1], chain_readlane(cq[q + 1], kk), c1); } \
      if constexpr ((P) % 2) col = chain_fma(-cq[P - 1], chain_readlane(cq[P - 1], kk), col);                        \
      col = col + c1; }                                                                                          \
    const float d = chain_readlane(col, kk);                                                                    \
    const float rs = chain_rsq(d);                                                                        \
    diag = chain_at_lane(lane, kk, d, diag);                                                                           \
    const F cp = chain_at_lane(lane, kk, 0.f, col * rs);                                                           \
    b = chain_fma(-cp, chain_readlane(b, kk) * rs, b);                                                               \
    cq[P] = cp;                                                                                             \
  }
#define NMF_DUAL_PIVOT8(P) NMF_DUAL_PIVOT(P) NMF_DUAL_PIVOT(P + 1) NMF_DUAL_PIVOT(P + 2) NMF_DUAL_PIVOT(P + 3) NMF_DUAL_PIVOT(P + 4) NMF_DUAL_PIVOT(P + 5) NMF_DUAL_PIVOT(P + 6) NMF_DUAL_PIVOT(P + 7)
#define NMF_DUAL_PIVOT4(P) NMF_DUAL_PIVOT(P) NMF_DUAL_PIVOT(P + 1) NMF_DUAL_PIVOT(P + 2) NMF_DUAL_PIVOT(P + 3)
  // an entry of the chain: who falls into it leaves a copy of b, who resumes there picks it up
#define NMF_DUAL_ENTRY(P) if constexpr (KEEP >= P) bsnap[P / kDualSnap] = b; case P: if constexpr (KEEP >= P) b = bsnap[P / kDualSnap];
  switch (KEEP > 0 ? start : 0) {
  default:
  NMF_DUAL_PIVOT4(0) NMF_DUAL_ENTRY(4) NMF_DUAL_PIVOT4(4) NMF_DUAL_ENTRY(8) NMF_DUAL_PIVOT4(8) NMF_DUAL_ENTRY(12) NMF_DUAL_PIVOT4(12) NMF_DUAL_ENTRY(16)
  NMF_DUAL_PIVOT8(16) NMF_DUAL_PIVOT8(24) NMF_DUAL_PIVOT8(32) NMF_DUAL_PIVOT8(40) NMF_DUAL_PIVOT8(48) NMF_DUAL_PIVOT8(56)
  }
#undef NMF_DUAL_ENTRY
#undef NMF_DUAL_PIVOT4
#undef NMF_DUAL_PIVOT8
#undef NMF_DUAL_PIVOT
}

}  // namespace nmf
