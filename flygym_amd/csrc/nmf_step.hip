// nmf_step.hip — the fused per-step physics kernel (gfx950, one wavefront per fly).
//
// Reference path replaced: mujoco_warp.step(m, d), the single call behind
// flygym.warp.GPUSimulation.step (reference src/flygym/warp/simulation.py:260-263), which the
// reference runs as ~100 Warp/CUDA kernel launches per step with constraint buffers in HBM
// (njmax = nconmax = 500 per world, :54-55).  Here the whole step — and any number of
// consecutive steps — is ONE launch; nothing but the fly's state (qpos, qvel, ctrl,
// warm-start) crosses HBM.
//
// Algorithmic design (MI355X-first, not a translation of MuJoCo's data flow):
//   * all spatial quantities are expressed in world axes about the root-body origin, so no
//     per-link frame changes are needed along a leg;
//   * no mass matrix and no constraint Jacobian are ever formed.  J·x is the velocity of the
//     contact point under body twists, Jᵀf is a wrench pushed down the chain, and every linear
//     solve (M⁻¹, (M + JᵀDJ)⁻¹ in the Newton solver, (M + hB)⁻¹ in the Euler step) is an O(n)
//     articulated-body sweep whose 6x6 articulated inertias absorb the active contact rows
//     (D·l lᵀ with l = [r x d; d]) — algebraically identical to factorising the nv x nv matrix
//     (124 kFLOP dense) at ~7 kFLOP, all in registers/LDS;
//   * the constraint problem, its Newton iterations and exact line search follow the oracle
//     (oracle/nmf_oracle.c) step for step, so results agree to float rounding.
#include "nmf_device.h"

namespace nmf {

// Stage boundaries.  One wave per workgroup, and the LDS unit takes a wave's operations in order: a read that follows
// another lane's write in program order sees it, so a boundary only has to order the accesses for the COMPILER — a
// wavefront-scope fence.  __syncthreads() (the round-1/2 behaviour) additionally parks the wave on `s_waitcnt lgkmcnt(0)`
// until its LDS writes have drained: ~60 times per step, 1.2 % of the launch.
#define WSYNC() do { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)
// NMF_TOPO_MASK (development builds only: `scripts/build_variant.sh x -DNMF_TOPO_MASK=1` compiles the LEGS_ONLY kernels alone,
// in a sixth of the time): bit k keeps the kernels of topology k (0 LEGS_ONLY, 1 LEGS_ACTIVE_ONLY, 2 / 3 general tree,
// 4 ALL_BIOLOGICAL, 5 ALL_POSSIBLE).  The shipped library has all of them.
#ifndef NMF_TOPO_MASK
#define NMF_TOPO_MASK 0x3f
#endif
#define NMF_HAS_TOPO(k) ((NMF_TOPO_MASK >> (k)) & 1)
constexpr float kNoiseFactor = 8.f;
// SolveReport: how the constraint solve of a step ended — one bit per kind, counted per world in stats_sum columns 4..15 (bit k ->
// column 4 + k; include/nmf.h) and, for the launch's last step, in stats column 4 (the bits) / 5 (pivots) / 6 (KKT residual).
// FlyLds::iters carries it: iterations | bits << 8 | most pivots of an elimination << 20.
enum : unsigned int {
  kExitDual = 1u << 8,         // solved in contact space (nmf_dual.h) — ended one of the five ways below:
  kExitKkt = 1u << 9,          //   the elimination's target satisfies its own active set: exact
  kExitTie = 1u << 10,         //   the pivot set of two eliminations ago again and what its target violates is small (1e-3 of the residuals)
  kExitStall = 1u << 11,       //   a fourth line search without measurable descent
  kExitCost = 1u << 12,        //   MuJoCo's improvement test / the cost's float32 rounding floor (from the sixth elimination on)
  kExitMaxIter = 1u << 13,     //   iteration limit
  kExitPrimal = 1u << 14,      // solved by the primal Newton loop (more contacts than the contact-space solve takes, a contact on the rest of the body, tether, general tree, fallback)
  kExitFallback = 1u << 15,    // the contact-space solve's end failed the residual test and the step was solved again on the primal loop
  kExitBigPivots = 1u << 16,   // an elimination had more pivots than live in registers without spilling (kDualRegPivots)
  kExitNoNoslip = 1u << 17,    // CPU flavour: a step with contacts that could not take the noslip pass
  kExitFree = 1u << 18,        // no contact: nothing to solve
};
constexpr int kExitKinds = 12;      // bits 8..19
constexpr int kDualRegPivots = 47;
// contact-space solves that do not end exactly: what the last target may violate, relative to the largest residual, before the step is
// solved again on the primal loop (the tie rule's own bound)
constexpr float kDualResidMax = 1e-3f;
constexpr int kDualExitFrom = 5;     // first elimination at which the contact-space solve's cost-based guards apply (nmf_dual.h)

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
#else
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

// tree tables staged in LDS once per launch (bodies in breadth-first order; see nmf_capi.hip): body of BFS slot k, parent /
// first dof / dof count / child range of body b, body of dof j, level starts
// (sized for the bodies / dofs the tree sweeps touch: everything for the tree kernels, root + rest for the hybrid ones —
// the hybrid kernel sits 700 bytes below the LDS budget of 5 flies per CU)
#define NMF_TREE_TABLES                                                                                                  \
  unsigned char t_body[TP::kTblB], t_parent[TP::kTblB], t_dofadr[TP::kTblB], t_dofnum[TP::kTblB], t_cstart[TP::kTblB],    \
      t_ccount[TP::kTblB], t_dofbody[TP::kTblV];                                                                          \
  unsigned char t_lvl[18], t_nlevel;

// LDS used by the general-tree sweeps only (nmf_tree.h)
template <class TP, bool STAR = TP::kStar, bool REST = (TP::kNFact > 1)>
struct TreeLds {};
template <class TP>
struct TreeLds<TP, false, true> {
  float fact[TP::kNFact][8];  // articulated-body factors per dof: U (6), u, 1/D — written going up, read going down
  float slot[TP::kNSlot][27]; // articulated inertia (symmetric, 21) + bias wrench (6) a body hands to its parent
  int rt_nb, rt_nv;
  NMF_TREE_TABLES
};
template <class TP>
struct TreeLds<TP, true, true> {   // hybrid kernels: the same for the rest bodies only
  float fact[TP::kNFact][8];
  // (no slot array: what a rest body hands to its parent lives only while an elimination sweep runs, in LDS that is dead
  // inside an articulated-body solve — FlyLds::slot_at.  2160 bytes: with a 64-control cap the ALL_BIOLOGICAL kernel fits
  // 8 flies per CU instead of 7.)
  // reduced constraint problem (physics_forward): while no rest body is in contact the rest's accelerations are
  // eliminated from the Newton loop — the root carries the rest's articulated inertia restA (symmetric 6x6) instead
  int reduced;
  float restA[21];
  unsigned int t_pack[kRestLevels][8][2];   // fast level passes: DevModel::rest_pack staged
  NMF_TREE_TABLES
};

// star kernels (register-bound at 8 flies per CU, LDS to spare) keep two row-fetch accelerators in LDS: the 3x3
// pyramid-coefficient matrix of every contact (c_m3) and every body's inertia as a symmetric 6x6 (Isym: six reads with
// lane-constant offsets that the compiler pairs into ds_read2); the hybrid kernels (LDS-bound) rebuild the former from
// the active-row mask and read inertia rows through InertiaRowMap
template <class TP> constexpr bool has_cm3() { if constexpr (TP::kStar) return TP::REST_B == 0; else return false; }
template <class TP> inline constexpr bool kHasCm3 = has_cm3<TP>();
template <class TP> inline constexpr bool kHasIsym = has_cm3<TP>();

// Row widths (in floats) of the per-dof motion subspaces S[NV][.] and the per-body twists / wrenches T, W[NB][.].  Six
// floats are used; the width decides the LDS banks.  In every chain sweep lane (leg g, component r) reads row
// (leg base + g * rows per leg), column r, so a 32-lane half of the wave (4 legs x 8 lanes) is conflict-free iff the four
// 6-bank windows at g * rows_per_leg * width (mod 32) do not overlap.  With width 6 the LEGS_ONLY strides are 66 and 48
// dwords = 2 and 16 (mod 32): up to 3 lanes per bank, 17-18 % of all LDS cycles were conflict cycles (profiles r1m,
// r2a).  Width 7 gives 77 = 13 and 56 = 24 (mod 32): disjoint windows.  Chosen per topology at compile time; the hybrid
// / tree kernels (LDS-bound) keep 6.
constexpr bool rows_conflict_free(int rows_per_leg, int width, int nleg) {
  const int ng = nleg < 4 ? nleg : 4;
  for (int a = 0; a < ng; ++a)
    for (int b = a + 1; b < ng; ++b) {
      const int d = (((b - a) * rows_per_leg * width) % 32 + 32) % 32;
      if (d < 6 || d > 26) return false;
    }
  return true;
}
constexpr int conflict_free_width(int rows_per_leg, int nleg) {
  for (int w = 6; w <= 9; ++w) if (rows_conflict_free(rows_per_leg, w, nleg)) return w;
  return 6;
}
template <class TP> constexpr int row_width_s() { if constexpr (TP::kStar) return TP::REST_B == 0 ? conflict_free_width(TP::NDL, TP::NLEG) : 6; else return 6; }
template <class TP> constexpr int row_width_tw() { if constexpr (TP::kStar) return TP::REST_B == 0 ? conflict_free_width(TP::NBL, TP::NLEG) : 6; else return 6; }
// Leg-chain kernels solve the constraints in contact space (nmf_dual.h) while a step has at most kDualMaxCon<TP> contacts.
// What LDS has to hold for it is G, the Gram matrix of the contacts' DIRECTION responses (normal and two tangents: three per
// contact, stored as one 3x3 block per unordered pair of contacts, dual_g_floats) — a pyramid row is n +- mu t, so an entry of
// A = J M^-1 J^T is four entries of G and three multiply-adds.  Two flavours:
//  * kDualS — stars without a rest-of-body tree (LEGS_ONLY, LEGS_ACTIVE_ONLY): factors on c_w + c_m3, G on Ib..W (the
//    inertias live a second time in Isym), warm start blended in, previous step's active set as first guess (act_hist);
//    16 contacts = 64 rows = the wave (G: 1224 floats; Ib..W of the 49-body skeleton: 1225);
//  * kDualH — hybrid kernels (ALL_BIOLOGICAL, ALL_POSSIBLE): no LDS to spare, so the leg factors go to vA..vD — or, where
//    they do not fit those either (ALL_POSSIBLE, kDualGlob), to the workgroup's scratch in HBM —, the root's, the rows'
//    reference accelerations and the hinge sums to c_w, G to T..W only (Ib is the one copy of the inertias: 13 contacts),
//    no warm-start term.  Steps with a contact on the rest of the body take the primal loop.
// One kernel per skeleton and world kind whatever the batch size: a world's result does not depend on how many worlds step
// beside it (rounds 3-4 had a second LEGS_ONLY flavour for small batches, nmf::Wide, because A's row triangle for 16 contacts
// cost two flies per CU).
template <class TP> constexpr bool dual_hybrid() {
  if constexpr (TP::kStar) return TP::REST_B > 0; else return false;
}
// ... whose leg factors (8 floats per leg hinge) do not fit the four solver vectors either (ALL_POSSIBLE: 144 leg hinges, 4.6 KB):
// they go to a scratch of the workgroup in HBM (DevState::dual_scratch) — written once per step by the smooth solve, read
// twice by the contact-space solve (response sweep, final expansion); a persistent workgroup's 4.6 KB stay in L2
template <class TP> constexpr bool dual_global() {
  if constexpr (TP::kStar) return TP::REST_B > 0 && 4 * TP::NV < TP::NLEG * TP::NDL * 8; else return false;
}
template <class TP> inline constexpr bool kDualS = has_cm3<TP>();
template <class TP> inline constexpr bool kDualH = dual_hybrid<TP>();
template <class TP> inline constexpr bool kDual = kDualS<TP> || kDualH<TP>;
template <class TP> inline constexpr bool kDualGlob = kDualH<TP> && dual_global<TP>();
constexpr int kDualScratchFloats = 8 * 6 * 24;      // per workgroup: the leg factors of the largest skeleton (six legs of 24 hinges)
constexpr int dual_g_floats(int ncon) { return 9 * ncon * (ncon + 1) / 2; }      // one 3x3 block per unordered pair of contacts
template <class TP> constexpr int dual_max_con() {
  if constexpr (kDualH<TP>) {      // the contacts whose blocks fit T..W
    int n = 0;
    while (n < 16 && dual_g_floats(n + 1) <= 2 * TP::NB * 6) ++n;
    return n;
  } else return 16;      // 64 rows = the wave; their reference accelerations take 64 floats of vB(..vC)
}
template <class TP> inline constexpr int kDualMaxCon = dual_max_con<TP>();
// LDS words of the active-set history (the contact-space solve's first guess, DevState::act_hist).  kDualS: a table by geom,
// 16 bits per geom (4 contacts x 4 rows); kDualH (no LDS to spare: the ALL_BIOLOGICAL kernel sits exactly on 160 KB / 8): a list
// of five words, one 16-bit entry per contact for the first ten contacts of the last solved step — geom (8) | ordinal within
// the geom (2) | active rows (4) | valid (1) — which the rows search; later contacts start from their own sign pattern.
template <class TP> inline constexpr int kHistLds = kDualS<TP> ? kActHistWords : kDualH<TP> ? 5 : 0;
template <class TP, class M> __device__ __forceinline__ int hist_words(const M& m) {      // ... of them in use
  if constexpr (kDualS<TP>) return (m.ng + 1) / 2; else return kHistLds<TP>;
}
template <class TP> constexpr int dual_pad_floats() {
  if constexpr (kDualS<TP>) {
    constexpr int need = dual_g_floats(kDualMaxCon<TP>);      // G (nmf_dual.h)
    constexpr int have = TP::NB * 11 + 2 * TP::NB * (TP::REST_B == 0 ? conflict_free_width(TP::NBL, TP::NLEG) : 6);
    return need > have ? need - have : 0;
  } else return 0;
}

// What the non-inlined stages (kinematics, collision) need of the model, staged in LDS once per launch.  Inside a
// non-inlined function the model is a generic reference: every field would be a flat load (full memory latency, and the
// LDS counter waits with it) and every array access two dependent round trips (pointer, then value), re-issued after each
// LDS store the compiler cannot tell apart from it.  From here a pointer costs one LDS read and the arrays are read as
// global memory.
struct HotModel {
  const float *dof_axis, *body_pos, *body_quat, *geom_p0, *geom_p1, *geom_radius, *geom_bsphere, *hull_vert, *pair_margin;
  const int *geom_body, *geom_type, *geom_hulladr, *geom_hullnum;
  float plane[4], terrain[5], hull_skin;
  int terrain_type, ng, sem_max_hull_contacts, terrain_walls;
};
template <class TP> struct FlyLds;
template <class TP> struct AbaHandoff;
template <class T> using gptr = const __attribute__((address_space(1))) T*;
template <class T> __device__ __forceinline__ gptr<T> G(const T* p) { return (gptr<T>)p; }
__device__ __forceinline__ V3 ld3(gptr<float> p) { return V3{p[0], p[1], p[2]}; }
__device__ __forceinline__ Q4 ldq(gptr<float> p) { return Q4{p[0], p[1], p[2], p[3]}; }

template <class TP>
struct __align__(16) FlyLds : TreeLds<TP> {
  // sizes: compile-time constants for the chain-star kernels, run-time values of the model for the tree kernel
  __device__ __forceinline__ int nv() const { if constexpr (TP::kStar) return TP::NV; else return this->rt_nv; }
  __device__ __forceinline__ int nb() const { if constexpr (TP::kStar) return TP::NB; else return this->rt_nb; }
  __device__ __forceinline__ int nq() const { return nv() + 1; }
  float qpos[TP::NQ + 3];
  float qvel[TP::NV], qacc[TP::NV];      // qacc doubles as the warm start
  // Body poses live from the kinematics stage to the end of the collision stage only (the pose outputs of a launch are
  // written right after its last collision stage), so they are overlaid on buffers that are dead in that window: the
  // rotation matrices of bodies 1.. on the six solver vectors, the positions of bodies 1.. on the contact wrenches.
  // The root's pose sits in the 9 / 3 floats in front of each region: it is read all step long (contact points are
  // relative to it) and `xmat()` / `xpos()` index all bodies uniformly.
  float xmat_root[9];
  // qacc_smooth .. vD are contiguous (6 NV floats): the velocity stage borrows them as one buffer
  float qacc_smooth[TP::NV], qfrc_smooth[TP::NV];
  float vA[TP::NV], vB[TP::NV], vC[TP::NV], vD[TP::NV];
  float ctrl[TP::kCtrl];
  float S[TP::NV][row_width_s<TP>()];
  // spatial inertia about the root origin: m, h, I (inertia * twist products; ABA rows via InertiaRowMap).  Rows are 11
  // floats apart where LDS allows: lane = body loops then hit 32 different banks (stride 10: bodies b and b + 16 collide)
  float Isym[kHasIsym<TP> ? TP::NB : 1][kHasIsym<TP> ? 21 : 1];   // the same as a symmetric 6x6 (upper triangle): row fetches of the star ABA
  // (Ib, T, W are contiguous and 16-byte aligned: the contact-space solve (nmf_dual.h) keeps the Gram matrix of the contact directions there)
  alignas(kDualS<TP> ? 16 : 4) float Ib[TP::NB][kHasCm3<TP> ? 11 : 10];
  static_assert(6 * TP::NV >= 9 * (TP::NB - 1), "rotation matrices do not fit the solver vectors");
  static_assert(7 * kMaxCon >= 3 * (TP::NB - 1), "body positions do not fit the contact wrenches");
  __device__ __forceinline__ float (*xmat())[9] { return reinterpret_cast<float(*)[9]>(&xmat_root[0]); }
  __device__ __forceinline__ const float (*xmat() const)[9] { return reinterpret_cast<const float(*)[9]>(&xmat_root[0]); }
  __device__ __forceinline__ float (*xpos())[3] { return reinterpret_cast<float(*)[3]>(&xpos_root[0]); }
  __device__ __forceinline__ const float (*xpos() const)[3] { return reinterpret_cast<const float(*)[3]>(&xpos_root[0]); }
  // body twists / wrenches, contiguous (12 NB floats).  Velocities live in W until the bias stage; the
  // kinematics stage borrows T..W for relative transforms; the ABA borrows it for its leg -> root hand-off
  float T[TP::NB][row_width_tw<TP>()], W[TP::NB][row_width_tw<TP>()];
  float dual_pad[dual_pad_floats<TP>()];      // what the contact-space solve's scratch needs beyond Ib..W (skeletons with few bodies)
  // dof_armature / dof_damping, staged once per launch.  The LDS-bound kernels (hybrid, tree) keep only the armature:
  // damping enters one passive-force pass and the Euler solve of a step, which read it from the model (dof_damp())
  float arm[TP::NV], damp[kHasCm3<TP> ? TP::NV : 1];
  float dlt[kHasCm3<TP> ? TP::NV : 1];   // armature + timestep * damping: the diagonal term of the Euler step's solve (star kernels)
  float c_r[kMaxCon][3], c_D[kMaxCon], c_mu[kMaxCon];   // c_D holds the distance until setup
  int c_info[kMaxCon];                  // geom | (leg sensor + 1) << 8 | body << 12 | active-row mask << 20
  alignas(kDualS<TP> ? 16 : 4) float xpos_pad_[kDualS<TP> ? 1 : 0];
  float xpos_root[3];
  // (c_w, c_m3 are contiguous and 16-byte aligned: between the smooth solve and the end of the contact-space solve they hold
  // the articulated-body factors of the mass matrix, DualFactors)
  float c_w[kMaxCon][7];     // contact wrenches (6 used; odd stride: lane = contact stores hit 32 different banks)
  // star kernels: the 3x3 pyramid-coefficient matrix of every contact for its active rows (nn, n1, n2, 11, 22), written
  // with the active-row mask; the hybrid kernels have no LDS to spare and rebuild it from the mask
  float c_m3[kHasCm3<TP> ? kMaxCon : 1][kHasCm3<TP> ? 5 : 1];
  // per row index r of a 6x6 (staged once per launch): [0..10] KLane constants of the contact stiffness rows; [11..13]
  // the row's map into a body's 10-float inertia (byte offsets of columns 0-2 / 3-5, 2-bit signs + 1): see InertiaRowMap
  // [14..19]: offsets of the row's six entries inside a packed symmetric 6x6 (ints).  The launch-constant conveniences
  // from here to `axis` exist in the star kernels with LDS to spare only: the hybrid / tree kernels are LDS-bound (one
  // more 512-byte granule is one fly per CU less) and derive the same values from the model when they need them.
  float k_tab[6][kHasIsym<TP> ? 20 : 14];
  float frame9[kHasIsym<TP> ? 9 : 1];   // contact frame of the ground plane (n, t1, t2), staged once per launch
  std::conditional_t<kHasIsym<TP>, HotModel, char> hot;
  float axis[kHasIsym<TP> ? TP::NV : 1][3];   // joint axes in their bodies' frames (star kernels with LDS to spare)
  float weldD[6], weld_w[6];            // tether weld: row stiffness 1/R and row wrench (zero without a tether)
  // first contact of every body (contacts are sorted by body; <= kMaxCon): ints for the star kernels (the ABA fetches a
  // leg's nine in paired reads), bytes where LDS is what limits residency
  using cstart_t = std::conditional_t<kHasIsym<TP>, int, unsigned char>;
  cstart_t body_cstart[(TP::NB + 1 + 3) / 4 * 4];
  // What rest body k (breadth-first slot) hands to its parent during an elimination sweep: articulated inertia (symmetric,
  // 21) + bias wrench (6).  Tree kernels keep an array; the hybrid kernels (LDS-bound) put the first 12 on the contact
  // wrenches and the others behind the leg -> root hand-off in T..W — both dead while an articulated-body solve runs.
  __device__ __forceinline__ float* slot_at(int k) {
    if constexpr (TP::kStar) {
      constexpr int kInCw = 7 * kMaxCon / 27;
      static_assert(TP::REST_B == 0 || (TP::REST_B - kInCw) * 27 * sizeof(float) + sizeof(AbaHandoff<TP>) <= sizeof(float) * TP::NB * 2 * row_width_tw<TP>(),
                    "hand-off slots of the rest do not fit T..W");
      return k < kInCw ? &c_w[0][0] + 27 * k : &T[0][0] + sizeof(AbaHandoff<TP>) / sizeof(float) + 27 * (k - kInCw);
    } else return this->slot[k];
  }
  // the constraint solver's second warm start (DevState::act_hist), carried from step to step: 16 bits per geom
  unsigned int act_hist[kHistLds<TP>];
  float* dual_glob[kDualGlob<TP> ? 1 : 0];      // kDualGlob: this workgroup's leg-factor scratch in HBM (set once per launch)
  int ncon, overflow;
  int iters;                            // SolveReport: Newton iterations | how the solve ended << 8 | pivots << 20
  float solve_resid;                    // ... and what its last elimination's target violates (nmf_dual.h)
  int nwall;                            // contacts of this step that touch a terrain side face (frame id != 0)
  // LDS vectors addressed by id: non-inlined functions take ids, not pointers, so that every access stays a
  // ds_* instruction (a float* argument would be a generic pointer -> flat_load / flat_store)
  __device__ __forceinline__ float* vec(int id) {
    switch (id) {
      case 0: return qacc;
      case 1: return qacc_smooth;
      case 2: return qfrc_smooth;
      case 3: return vA;
      case 4: return vB;
      case 5: return vC;
      default: return vD;
    }
  }
};
// the staged copy where there is one, else the same fields gathered from the model
template <class TP> __device__ __forceinline__ HotModel hot_model(const FlyLds<TP>& s, const GModel& m) {
  if constexpr (kHasIsym<TP>) return s.hot;
  else {
    HotModel h;
    h.dof_axis = (const float*)m.dof_axis; h.body_pos = (const float*)m.body_pos; h.body_quat = (const float*)m.body_quat;
    h.geom_p0 = (const float*)m.geom_p0; h.geom_p1 = (const float*)m.geom_p1; h.geom_radius = (const float*)m.geom_radius;
    h.geom_bsphere = (const float*)m.geom_bsphere; h.hull_vert = (const float*)m.hull_vert; h.pair_margin = (const float*)m.pair_margin;
    h.geom_body = (const int*)m.geom_body; h.geom_type = (const int*)m.geom_type; h.geom_hulladr = (const int*)m.geom_hulladr;
    h.geom_hullnum = (const int*)m.geom_hullnum;
#pragma unroll
    for (int i = 0; i < 4; ++i) h.plane[i] = m.plane[i];
#pragma unroll
    for (int i = 0; i < 5; ++i) h.terrain[i] = m.terrain[i];
    h.hull_skin = m.hull_skin; h.terrain_type = m.terrain_type; h.ng = m.ng; h.sem_max_hull_contacts = m.sem_max_hull_contacts;
    h.terrain_walls = m.sem_terrain_walls;
    return h;
  }
}
template <class TP> __device__ __forceinline__ float dof_damp(const FlyLds<TP>& s, const GModel& m, int j) {
  if constexpr (kHasCm3<TP>) return s.damp[j]; else return m.dof_damping[j];
}
// diagonal term of an articulated-body solve: armature + hdamp * damping (hdamp = 0 except in the Euler step's solve)
template <class TP> __device__ __forceinline__ float dof_delta(const FlyLds<TP>& s, const GModel& m, int j, float hdamp) {
  if constexpr (kHasCm3<TP>) return (hdamp != 0.f ? s.dlt : s.arm)[j];        // hdamp is 0 or the timestep
  else return hdamp != 0.f ? fmaf(hdamp, m.dof_damping[j], s.arm[j]) : s.arm[j];
}
template <class TP> __device__ __forceinline__ int tbl_dofbody(const FlyLds<TP>& s, int j) { if constexpr (TP::kNFact > 1) return s.t_dofbody[j]; else return 0; }
template <class TP> __device__ __forceinline__ int tbl_dofadr(const FlyLds<TP>& s, int b) { if constexpr (TP::kNFact > 1) return s.t_dofadr[b]; else return 0; }
template <class TP> __device__ __forceinline__ int tbl_dofnum(const FlyLds<TP>& s, int b) { if constexpr (TP::kNFact > 1) return s.t_dofnum[b]; else return 0; }
enum { V_QACC = 0, V_QACC_SMOOTH = 1, V_QFRC_SMOOTH = 2, V_A = 3, V_B = 4, V_C = 5, V_D = 6 };

__device__ __forceinline__ int info_geom(int i) { return i & 0xff; }
__device__ __forceinline__ int info_sensor(int i) { return ((i >> 8) & 0xf) - 1; }
__device__ __forceinline__ int info_body(int i) { return (i >> 12) & 0xff; }
__device__ __forceinline__ int info_act(int i) { return (i >> 20) & 0xf; }
__device__ __forceinline__ int info_fid(int i) { return (i >> 24) & 0x7; }     // contact frame: 0 the ground plane's, 1..4 a terrain side face (+x, -x, +y, -y)
__device__ __forceinline__ int info_pack(int geom, int sensor, int body, int act) {
  return geom | ((sensor + 1) << 8) | (body << 12) | (act << 20);
}

// ABA leg -> root hand-off, overlaid on the T..W region (free while an ABA sweep runs)
template <class TP>
struct AbaHandoff {
  float legIA[TP::NLEG][6][6], legpA[TP::NLEG][6], rootA[6][6], rootb[6];
};

struct Frame { V3 n, t1, t2; };

template <class LDS> __device__ __forceinline__ Frame ld_frame(const LDS& s, const GModel& m);
__device__ __forceinline__ Frame make_frame(V3 n) {
  V3 t = fabsf(n.y) < 0.5f ? v3(0.f, 1.f, 0.f) : v3(0.f, 0.f, 1.f);
  float dn = dot(t, n);
  V3 t1 = t - dn * n;
  float l = sqrtf(dot(t1, t1));
  t1 = (1.0f / l) * t1;
  return Frame{n, t1, cross(n, t1)};
}

template <class LDS> __device__ __forceinline__ Frame ld_frame(const LDS& s, const GModel& m) {
  if constexpr (sizeof(s.frame9) == 9 * sizeof(float)) return Frame{ld3(&s.frame9[0]), ld3(&s.frame9[3]), ld3(&s.frame9[6])};
  else return make_frame(v3(m.plane[0], m.plane[1], m.plane[2]));
}

// Frame of a contact: the ground plane's (fid 0) or that of a terrain side face with outward normal +x, -x, +y, -y (fid
// 1..4: make_frame of that axis, written out).  Branch-free: lanes of a wave may hold contacts of different faces.
__device__ __forceinline__ Frame contact_frame(int fid, const Frame& f0) {
  const float sg = (fid & 1) ? 1.f : -1.f;
  const bool xw = fid <= 2, pl = fid == 0;
  Frame f;
  f.n = pl ? f0.n : (xw ? v3(sg, 0.f, 0.f) : v3(0.f, sg, 0.f));
  f.t1 = pl ? f0.t1 : (xw ? v3(0.f, 1.f, 0.f) : v3(0.f, 0.f, 1.f));
  f.t2 = pl ? f0.t2 : (xw ? v3(0.f, 0.f, sg) : v3(sg, 0.f, 0.f));
  return f;
}

template <class TP>
__device__ __forceinline__ int dof_body_of(int j) {
  if (j < 6) return 0;
  const int leg = (j - TP::LD0) / TP::NDL, d = (j - TP::LD0) % TP::NDL;     // leg dofs only (j >= LD0)
  int lb = 0;
  static_for<TP::NBL - 1>([&](auto I) { constexpr int l = decltype(I)::value; lb += d >= TP::first_dof(l + 1) ? 1 : 0; });
  return TP::LB0 + leg * TP::NBL + lb;
}

// ------------------------------------------------------------------ lane roles
struct LaneRole {
  int grp, r, lg, rr;
  bool live;      // a real (leg, component) lane
  float mask;     // 1 for r < 6 else 0 (zero contribution to group sums)
};
template <class TP>
__device__ __forceinline__ LaneRole lane_role(int lane) {
  LaneRole L;
  L.grp = lane >> 3; L.r = lane & 7;
  L.lg = L.grp < TP::NLEG ? L.grp : TP::NLEG - 1;
  L.rr = L.r < 6 ? L.r : 5;
  L.live = L.grp < TP::NLEG && L.r < 6;
  L.mask = L.r < 6 ? 1.f : 0.f;
  return L;
}

// general-tree sweeps (nmf_tree.h, included at the end of this file)
template <class TP> __device__ void tree_kinematics_chain(FlyLds<TP>& s, const GModel& m, int lane, float (*relm)[12]);
template <class TP> __device__ void tree_velocity_bias(FlyLds<TP>& s, const GModel& m, int lane);
template <class TP> __device__ void tree_sweep_twists(FlyLds<TP>& s, const float* x, float (*T)[row_width_tw<TP>()], const GModel& m, int lane);
template <class TP, class Extra, class Emit>
__device__ __forceinline__ void tree_sweep_project(FlyLds<TP>& s, float (*W)[row_width_tw<TP>()], const GModel& m, int lane, Extra&& extra, Emit&& emit);
template <class TP, bool WELD>
__device__ void tree_aba_solve(FlyLds<TP>& s, int tau_id, int x_id, bool withK, float hdamp, const GModel& m, int lane);
template <class TP> __device__ void tree_velocity_bias_levels(FlyLds<TP>& s, const GModel& m, int lane);
template <class TP> __device__ void tree_sweep_twists_levels(FlyLds<TP>& s, const float* x, float (*T)[row_width_tw<TP>()], const GModel& m, int lane);
template <class TP, class Extra>
__device__ __forceinline__ void tree_gather_levels(FlyLds<TP>& s, float (*W)[row_width_tw<TP>()], const GModel& m, int lane, Extra&& extra);
template <class S, class F> __device__ __forceinline__ void tree_down(const S& s, int lane, F&& f);
template <class S, class F> __device__ __forceinline__ void tree_up(const S& s, int lane, F&& f);
struct Frame;
template <class TP, bool WELD>
__device__ __forceinline__ void tree_aba_eliminate_body(FlyLds<TP>& s, int b, const float* tau, bool withK, float hdamp,
                                                        const GModel& m, const Frame& fr);
template <class TP>
__device__ __forceinline__ void tree_aba_expand_body(FlyLds<TP>& s, int b, SV a, float* x, const GModel& m);
struct RestNode;
template <class TP, bool FAST, bool UP, class F> __device__ __forceinline__ void rest_levels(FlyLds<TP>& s, int lane, F&& f);
template <class TP, int NUM>
__device__ __forceinline__ void rest_aba_eliminate(FlyLds<TP>& s, const RestNode& nd, const float* tau, bool withK, float hdamp,
                                                   const Frame& fr, const LaneRole& L, const int (&so)[6], const struct InertiaRowMap& IM, const GModel& m);
template <class TP, int NUM, bool HOMOGENEOUS>
__device__ __forceinline__ void rest_aba_expand(FlyLds<TP>& s, const RestNode& nd, float* x, const LaneRole& L);

// ------------------------------------------------------------------ kinematics
template <class TP>
__device__ __noinline__ void stage_kinematics(FlyLds<TP>& s, const GModel& m, int lane) {
  // scratch (dead between steps): joint quaternions in the solver vectors, per-body relative
  // rotation matrices + offsets in the ABA hand-off buffer, body-frame hinge axes in T
  // Odd strides: lane = dof / lane = body loops and the leg groups of the chain pass (8 bodies apart) would otherwise
  // hit a bank every 8 lanes / all four groups of a half-wave the same bank (stride 4: 4-way, stride 12: 4-way).
  constexpr int kJq = 5;                                                 // NV x 5 floats in qacc_smooth .. vD (6 NV floats)
  constexpr int kRel = row_width_tw<TP>() > 6 ? 13 : 12;     // 13 needs the wide T / W rows (star kernels without rest bodies)
  float(*jq)[kJq] = reinterpret_cast<float(*)[kJq]>(&s.qacc_smooth[0]);
  float(*relm)[kRel] = reinterpret_cast<float(*)[kRel]>(&s.T[0][0]) - 1;  // bodies 1..NB-1: (NB-1) x kRel floats in T..W
  float(*axb)[3] = reinterpret_cast<float(*)[3]>(&s.Ib[0][0]);          // NV x 3 floats (Ib is rebuilt afterwards)
  static_assert((TP::NB - 1) * kRel <= TP::NB * 2 * row_width_tw<TP>() && TP::NV * 3 <= TP::NB * 10 && kJq <= 6, "kinematics scratch does not fit");
  const HotModel hmk = hot_model(s, m);
  const gptr<float> g_axis = G(hmk.dof_axis), g_quat = G(hmk.body_quat), g_pos = G(hmk.body_pos);
  auto axis_of = [&](int j) { if constexpr (kHasIsym<TP>) return ld3(s.axis[j]); else return ld3(g_axis + 3 * j); };
  for (int j = 6 + lane; j < s.nv(); j += kWave) {
    float sn, cs;
    sincos_bounded(0.5f * s.qpos[j + 1], &sn, &cs);
    const V3 ax = axis_of(j);
    jq[j][0] = cs; jq[j][1] = ax.x * sn; jq[j][2] = ax.y * sn; jq[j][3] = ax.z * sn;
  }
  if (lane == 0) {
    Q4 q = qnorm(ldq(&s.qpos[3]));
    st3(s.xpos()[0], ld3(&s.qpos[0]));
    qmat(s.xmat()[0], q);
  }
  WSYNC();
  for (int b = 1 + lane; b < s.nb(); b += kWave) {
    int adr, num;
    if constexpr (TP::kStar) {
      if (b >= TP::LB0) {
        const int lb = (b - TP::LB0) % TP::NBL;
        adr = TP::LD0 + ((b - TP::LB0) / TP::NBL) * TP::NDL; num = 0;
        static_for<TP::NBL>([&](auto I) { constexpr int l = decltype(I)::value; if (lb == l) { adr += TP::first_dof(l); num = TP::dofs(l); } });
      } else { adr = tbl_dofadr(s, b); num = tbl_dofnum(s, b); }     // hybrid: the rest of the body (tree part)
    } else { adr = tbl_dofadr(s, b); num = tbl_dofnum(s, b); }
    const Q4 bq = ldq(g_quat + 4 * b);
    const V3 bp = ld3(g_pos + 3 * b);
    Q4 P = Q4{1.f, 0.f, 0.f, 0.f};
    for (int j = adr + num - 1; j >= adr; --j) {
      st3(axb[j], qrot_conj(P, axis_of(j)));
      P = qmul(ldq(jq[j]), P);
    }
    qmat(relm[b], qnorm(qmul(bq, P)));
    st3(&relm[b][9], bp);
  }
  WSYNC();
  if constexpr (!TP::kStar) tree_kinematics_chain(s, m, lane, relm);
  else {
    if constexpr (TP::REST_B > 0) tree_kinematics_chain(s, m, lane, relm);     // head, abdomen, wings, ...: tree levels
    // chain of rigid transforms down each leg: lane (leg, r < 3) carries row r of the rotation and
    // component r of the position:  R_b = R_parent * Rrel_b ,  p_b = p_parent + R_parent * off_b
    const LaneRole L = lane_role<TP>(lane);
    const int r3 = L.r < 3 ? L.r : 2;
    float R0 = s.xmat()[0][3 * r3], R1 = s.xmat()[0][3 * r3 + 1], R2 = s.xmat()[0][3 * r3 + 2];
    float p = s.xpos()[0][r3];
    const int b0 = TP::LB0 + L.lg * TP::NBL;
    // the relative transform of level l + 1 is requested before level l's results are stored: its LDS round trip runs
    // under the stores (the compiler keeps the loads behind them otherwise — it cannot tell the two regions apart)
    float Mn[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) Mn[k] = relm[b0][k];
    static_for<TP::NBL>([&](auto I) {
      constexpr int l = decltype(I)::value;
      float M[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) M[k] = Mn[k];
      p += R0 * M[9] + R1 * M[10] + R2 * M[11];
      const float n0 = R0 * M[0] + R1 * M[3] + R2 * M[6];
      const float n1 = R0 * M[1] + R1 * M[4] + R2 * M[7];
      const float n2 = R0 * M[2] + R1 * M[5] + R2 * M[8];
      R0 = n0; R1 = n1; R2 = n2;
      if constexpr (l + 1 < TP::NBL) {
#pragma unroll
        for (int k = 0; k < 12; ++k) Mn[k] = relm[b0 + l + 1][k];
        __builtin_amdgcn_sched_barrier(0);
      }
      s.xmat()[b0 + l][3 * r3] = R0; s.xmat()[b0 + l][3 * r3 + 1] = R1; s.xmat()[b0 + l][3 * r3 + 2] = R2;
      s.xpos()[b0 + l][r3] = p;
    });
  }
  WSYNC();
  for (int j = lane; j < s.nv(); j += kWave) {
    SV S;
    if (j < 3) {
      S.a = v3(0.f, 0.f, 0.f);
      S.l = v3(j == 0 ? 1.f : 0.f, j == 1 ? 1.f : 0.f, j == 2 ? 1.f : 0.f);
    } else if (j < 6) {
      int c = j - 3;
      S.a = v3(s.xmat()[0][c], s.xmat()[0][3 + c], s.xmat()[0][6 + c]);
      S.l = v3(0.f, 0.f, 0.f);
    } else {
      int b;
      if constexpr (TP::kStar) b = j >= TP::LD0 ? dof_body_of<TP>(j) : tbl_dofbody(s, j); else b = tbl_dofbody(s, j);
      V3 a = mat_vec(s.xmat()[b], ld3(axb[j]));
      V3 r = ld3(s.xpos()[0]) - ld3(s.xpos()[b]);
      S.a = a;
      S.l = cross(a, r);
    }
    stsv(s.S[j], S);
  }
  WSYNC();
}

template <class TP>
__device__ void stage_inertia(FlyLds<TP>& s, const GModel& m, int lane) {
  for (int b = lane; b < s.nb(); b += kWave) {
    const float* R = s.xmat()[b];
    const float* q = &m.body_inertia[6 * b];
    float Il[9] = {q[0], q[3], q[4], q[3], q[1], q[5], q[4], q[5], q[2]};
    float Tm[9], Iw[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) Tm[3 * i + j] = R[3 * i] * Il[j] + R[3 * i + 1] * Il[3 + j] + R[3 * i + 2] * Il[6 + j];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) Iw[3 * i + j] = Tm[3 * i] * R[3 * j] + Tm[3 * i + 1] * R[3 * j + 1] + Tm[3 * i + 2] * R[3 * j + 2];
    V3 c = mat_vec(R, ld3(&m.body_ipos[3 * b])) + (ld3(s.xpos()[b]) - ld3(s.xpos()[0]));
    float ms = m.body_mass[b], cc = dot(c, c);
    float* I = s.Ib[b];
    I[0] = ms; I[1] = ms * c.x; I[2] = ms * c.y; I[3] = ms * c.z;
    I[4] = Iw[0] + ms * (cc - c.x * c.x); I[5] = Iw[4] + ms * (cc - c.y * c.y); I[6] = Iw[8] + ms * (cc - c.z * c.z);
    I[7] = Iw[1] - ms * c.x * c.y; I[8] = Iw[2] - ms * c.x * c.z; I[9] = Iw[5] - ms * c.y * c.z;
    if constexpr (kHasIsym<TP>) {
      float* Q = s.Isym[b];                // [[I, [h]x], [-[h]x, m 1]], upper triangle row-major
      Q[0] = I[4]; Q[1] = I[7]; Q[2] = I[8]; Q[3] = 0.f;   Q[4] = -I[3]; Q[5] = I[2];
      Q[6] = I[5]; Q[7] = I[9]; Q[8] = I[3]; Q[9] = 0.f;   Q[10] = -I[1];
      Q[11] = I[6]; Q[12] = -I[2]; Q[13] = I[1]; Q[14] = 0.f;
      Q[15] = ms; Q[16] = 0.f; Q[17] = 0.f; Q[18] = ms; Q[19] = 0.f; Q[20] = ms;
    }
  }
  WSYNC();
}

// ------------------------------------------------------------------ collision (geom vs ground plane)
// piecewise-constant ground height under (x, y): build-defined terrains (oracle: terrain_height)
__device__ __forceinline__ float terrain_kind(int kind, float p0, float p1, float p2, float x, float y) {
  if (kind == 1) { const float period = p0 + p1; const float u = x - floorf(x / period) * period; return u < p0 ? 0.f : -p2; }
  if (kind == 2) { const float i = floorf(x / p0), j = floorf(y / p0); const float sum = i + j;
                   const float par = sum - 2.f * floorf(sum / 2.f); return par != 0.f ? p1 : 0.f; }
  return 0.f;
}
__device__ __forceinline__ float terrain_height(int terrain_type, const float* p, float x, float y) {
  if (terrain_type == 3) {
    const float st = floorf(x / p[3]); const float k = st - 3.f * floorf(st / 3.f);
    return k == 1.f ? terrain_kind(1, 1.0f, p[1], p[2], x, y) : (k == 2.f ? terrain_kind(2, p[0], 0.35f, 0.f, x, y) : 0.f);
  }
  return terrain_kind(terrain_type, p[0], p[1], p[2], x, y);
}

// The terrain as boxes (oracle: cell_bounds / terrain_probe; specification: flygym_amd/compose/world.py::terrain_probe).
// Bounds (x_lo, x_hi, y_lo, y_hi) of a constant-height cell; +-kFar where the lattice does not divide that axis.
constexpr float kFar = 1e30f;
constexpr float kProbeEps = 1e-4f;
constexpr float kOneCell = 0.02f;     // clearance [mm] of a footprint from its cell's boundary for the one-cell paths of the collision stage
// Height and bounds of the cell that holds (x, y) in one go (the same expressions as terrain_height and the oracle's
// cell_bounds: the lattice indices are shared)
__device__ __forceinline__ float terrain_cell_kind(int kind, float p0, float p1, float p2, float x, float y, float* b) {
  b[0] = -kFar; b[1] = kFar; b[2] = -kFar; b[3] = kFar;
  if (kind == 1) {
    const float period = p0 + p1; const float k = floorf(x / period); const float u = x - k * period;
    if (u < p0) { b[0] = k * period; b[1] = k * period + p0; return 0.f; }
    b[0] = k * period + p0; b[1] = (k + 1.f) * period; return -p2;
  }
  if (kind == 2) {
    const float i = floorf(x / p0), j = floorf(y / p0);
    b[0] = i * p0; b[1] = (i + 1.f) * p0; b[2] = j * p0; b[3] = (j + 1.f) * p0;
    const float sum = i + j; const float par = sum - 2.f * floorf(sum / 2.f);
    return par != 0.f ? p1 : 0.f;
  }
  return 0.f;
}
__device__ __forceinline__ float terrain_cell(int terrain_type, const float* p, float x, float y, float* b) {
  if (terrain_type == 3) {
    const float st = floorf(x / p[3]); const float k = st - 3.f * floorf(st / 3.f);
    const float h = k == 1.f ? terrain_cell_kind(1, 1.0f, p[1], p[2], x, y, b) : (k == 2.f ? terrain_cell_kind(2, p[0], 0.35f, 0.f, x, y, b)
                                                                                            : terrain_cell_kind(0, 0.f, 0.f, 0.f, x, y, b));
    const float lo = st * p[3], hi = (st + 1.f) * p[3];
    if (b[0] < lo) b[0] = lo;
    if (b[1] > hi) b[1] = hi;
    return h;
  }
  return terrain_cell_kind(terrain_type, p[0], p[1], p[2], x, y, b);
}
// One collision probe (point, rho = 0, or sphere of radius rho) at (x, y), height zc over the ground plane: dtop = signed
// distance of its lowest point to the top of its cell (kFar: it is inside that box and leaves it sideways), dwall / wall
// = signed distance to the nearest side face that concerns it and the face's code 1..4 (outward normal +x, -x, +y, -y).
// `reach`: faces further than that from the probe's surface cannot make a contact (the pair's margin) — a probe above its
// cell with no boundary within reach returns without looking at the neighbours (nearly every hull vertex).
__device__ __forceinline__ void terrain_probe(int terrain_type, const float* p, bool walls, float x, float y, float zc, float rho,
                                              float reach, float& dtop, float& dwall, int& wall) {
  float b[4];
  const float h0 = terrain_cell(terrain_type, p, x, y, b);
  const float zb = zc - rho;
  dtop = zb - h0; dwall = kFar; wall = 0;
  if (!walls) return;
  const float delta[4] = {b[1] - x, x - b[0], b[3] - y, y - b[2]};
  if (zb >= h0 && fminf(fminf(delta[0], delta[1]), fminf(delta[2], delta[3])) - rho > reach) return;
  // The neighbour across boundary e matters only if its face is within reach of the probe, or — for a probe inside its
  // own cell's box — if that boundary is nearer than the way out through the top: the others are never looked up (a
  // lattice evaluation each; a hull vertex next to one edge of its cell needs one of the four).  A face further than
  // `reach` is reported as no face at all (dwall = kFar): no caller uses a larger distance.
  const float pen0 = h0 - zb;
  float he[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    he[e] = h0;
    if (delta[e] < kFar && (delta[e] - rho <= reach || (zb < h0 && delta[e] + rho < pen0)))
      he[e] = e == 0 ? terrain_height(terrain_type, p, b[1] + kProbeEps, y) : e == 1 ? terrain_height(terrain_type, p, b[0] - kProbeEps, y)
            : e == 2 ? terrain_height(terrain_type, p, x, b[3] + kProbeEps) : terrain_height(terrain_type, p, x, b[2] - kProbeEps);
  }
  // Neighbours that reach above the probe's lowest point.  Centre below the neighbour's top (every point probe): its side
  // face, codes 2, 1, 4, 3 (the face's normal is -e).  Centre above it by v < rho: the sphere reaches over the top EDGE —
  // nearer the face (delta >= v) it is still the face, otherwise the neighbour's top carries it (normal +z): the depth
  // stays continuous when a capsule end rolls off a cell's edge.
  float edge_top = kFar;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (!(delta[e] - rho <= reach && he[e] > zb)) continue;
    if (zc - he[e] > delta[e]) edge_top = fminf(edge_top, zb - he[e]);
    else if (delta[e] - rho < dwall) { dwall = delta[e] - rho; wall = (e ^ 1) + 1; }
  }
  if (zb < h0) {
    float pen = h0 - zb; int code = 0;   // inside its own cell's box: the ways out (codes 1..4: the normal is +e)
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (delta[e] < kFar && he[e] <= zb && delta[e] + rho < pen) { pen = delta[e] + rho; code = e + 1; }
    if (code) { dtop = kFar; if (-pen < dwall) { dwall = -pen; wall = code; } }
  }
  dtop = fminf(dtop, edge_top);
}

// Scratch of the collision stage, overlaid on the T..W region (free between steps)
struct CollisionScratch {
  float r[kMaxCon][3], dist[kMaxCon];
  int info[kMaxCon];       // geom | k << 8 | body << 12 | frame id << 20   (k-th contact of that hull)
};

__device__ __forceinline__ float readlane_f(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

// ROUGH: the world has a terrain (height cells with side faces); flat worlds run the instantiation without any of it
template <class TP, bool ROUGH>
__device__ __noinline__ void stage_collision(FlyLds<TP>& s, const GModel& m, int lane) {
  static_assert(sizeof(CollisionScratch) <= sizeof(float) * TP::NB * 12, "collision scratch does not fit T..W");
  CollisionScratch& X = *reinterpret_cast<CollisionScratch*>(&s.T[0][0]);
  // first contact slot of every geom (up to 128 ints): behind the scratch in T..W where that is large enough, else behind
  // the body positions in the contact-wrench buffer (both dead until the solver starts)
  constexpr bool kSlotInTW = sizeof(CollisionScratch) + 2 * kWave * sizeof(int) <= sizeof(float) * TP::NB * 12;
  static_assert(kSlotInTW || 3 * (TP::NB - 1) + 2 * kWave <= 7 * kMaxCon, "slot table (128 geoms) does not fit");
  int* geom_slot0 = kSlotInTW ? reinterpret_cast<int*>(&s.T[0][0]) + sizeof(CollisionScratch) / sizeof(int)
                              : reinterpret_cast<int*>(&s.c_w[0][0]) + 3 * (TP::NB - 1);
  // terrains: the vertices of the hull being scanned that lie within the margin (index, distance), in index order — what
  // is left of T..W behind the scratch (and the slot table) holds kCand of them
  constexpr int kTwUsed = (int)sizeof(CollisionScratch) + (kSlotInTW ? 2 * kWave * (int)sizeof(int) : 0);
  constexpr int kCandRoom = ((int)sizeof(float) * TP::NB * 12 - kTwUsed) / 8;
  constexpr int kCand = kCandRoom > kWave ? kWave : kCandRoom;
  constexpr bool kListed = ROUGH && kCand >= 8;
  int* cand_idx = reinterpret_cast<int*>(&s.T[0][0]) + kTwUsed / 4;
  float* cand_d = reinterpret_cast<float*>(cand_idx + (kCand > 0 ? kCand : 0));
  // the model's side of this stage, staged in LDS at launch (see HotModel): scalars once, arrays as global memory
  const HotModel hm = hot_model(s, m);
  const int ng = hm.ng, terrain_type = hm.terrain_type, max_hull_contacts = hm.sem_max_hull_contacts;
  const bool walls = hm.terrain_walls != 0;
  const float hull_skin = hm.hull_skin, terrain_top = hm.terrain[4];
  const float tpar[4] = {hm.terrain[0], hm.terrain[1], hm.terrain[2], hm.terrain[3]};
  const gptr<int> geom_body = G(hm.geom_body), geom_type = G(hm.geom_type), geom_hulladr = G(hm.geom_hulladr),
                  geom_hullnum = G(hm.geom_hullnum);
  const gptr<float> pair_margin = G(hm.pair_margin), geom_bsphere = G(hm.geom_bsphere), geom_radius = G(hm.geom_radius),
                    geom_p0 = G(hm.geom_p0), geom_p1 = G(hm.geom_p1), hull_vert = G(hm.hull_vert);
  const V3 n = ld3(hm.plane);
  const float pd = hm.plane[3];
  const V3 o = ld3(s.xpos()[0]);
  constexpr bool rough = ROUGH;
  SUB_T0();
  // ---- phase 1, lane = geom: one batch of parameter loads, bounding-sphere cull, capsules resolved in place
  // (more than 64 contact geoms — e.g. every body segment in contact — take further passes of 64)
  int nh = 0, slot_base = 0;
  for (int g0 = 0; g0 < ng; g0 += kWave) {
  const int gi = g0 + lane;
  int g_body = 0, g_type = -1, g_hadr = 0, g_hnum = 0, cnt = 0;
  float g_margin = 0.f, cd0 = 0.f, cd1 = 0.f;
  V3 cp0 = v3(0, 0, 0), cp1 = v3(0, 0, 0);
  // terrains with side faces: a capsule end may also touch a face -> up to 4 contacts per capsule (ends x {top, face});
  // the two face contacts and the frame ids of all four (3 bits each) live here
  float cdw0 = 0.f, cdw1 = 0.f; V3 cpw0 = v3(0, 0, 0), cpw1 = v3(0, 0, 0); int cfid = 0, cntw = 0;
  bool near = false;
  // terrains: g_ttop = the highest cell top under the geom's footprint (bounding sphere + margin); one_cell: the footprint
  // lies inside ONE cell, further than kOneCell from its boundary — no vertex of it can meet a side face, and all of
  // them see the same top, g_ttop
  bool one_cell = false; float g_ttop = 0.f;
  if (gi < ng) {
    g_body = geom_body[gi]; g_type = geom_type[gi]; g_margin = pair_margin[gi];
    g_hadr = geom_hulladr[gi]; g_hnum = geom_hullnum[gi];
    const V3 bs = ld3(geom_bsphere + 4 * gi);
    const float bs_r = geom_bsphere[4 * gi + 3], rad = geom_radius[gi];
    const V3 l0 = ld3(geom_p0 + 3 * gi), l1 = ld3(geom_p1 + 3 * gi);
    const float* R = s.xmat()[g_body];
    const V3 xp = ld3(s.xpos()[g_body]);
    V3 cw = mat_vec(R, bs);
    float dc = dot(n, cw) + dot(n, xp) - pd;
    // Terrains: the ground under the geom is no higher than the highest cell its bounding sphere's footprint touches.
    // Against the global maximum every leg segment dangling in a 2 mm gap passed the cull: 21 hull scans per step on the
    // gapped world instead of 4.
    // The cell under the centre comes first: most footprints lie inside it (cells are 1 mm and more, a leg segment's
    // radius 0.1-0.3 mm) and need neither another look-up nor, later, a terrain probe per hull vertex.  Otherwise the
    // footprint's cells are walked along x from its low end — each cell's own high boundary leads to the next, so a cell
    // of any width is met (round 3 sampled 3 x 3 points a footprint radius apart and could step over a raised piece
    // narrower than that, e.g. where a stripe of the mixed terrain cuts a block) — and every one is read at three
    // heights of y, which meets all the blocks' rows unless a row is narrower than the radius (then: the global maximum).
    float ttop = terrain_top;
    const V3 p0 = mat_vec(R, l0) + xp, p1 = mat_vec(R, l1) + xp;
    if (rough && dc - bs_r - terrain_top <= g_margin) {
      // The footprint: the bounding sphere's box cut with the box of the bounding cylinder / the capsule itself (p0, p1, rad) —
      // a thin tarsal segment covers a strip, not the disc of its bounding sphere (round 4: on the blocks far fewer hulls
      // "straddle" a cell boundary, i.e. more take the one-cell path and fewer see a raised neighbour's top) — widened by
      // the margin: a face within the margin of a vertex belongs to a cell the footprint touches.
      const float cx = cw.x + xp.x, cy = cw.y + xp.y, fr = bs_r + g_margin, fc = rad + g_margin;
      const float fx0 = fmaxf(cx - fr, fminf(p0.x, p1.x) - fc), fx1 = fminf(cx + fr, fmaxf(p0.x, p1.x) + fc);
      const float fy0 = fmaxf(cy - fr, fminf(p0.y, p1.y) - fc), fy1 = fminf(cy + fr, fmaxf(p0.y, p1.y) + fc);
      const float mx = 0.5f * (fx0 + fx1), my = 0.5f * (fy0 + fy1);
      float cb[4];
      ttop = terrain_cell(terrain_type, tpar, mx, my, cb);
      const float clear = fminf(fminf(cb[1] - fx1, fx0 - cb[0]), fminf(cb[3] - fy1, fy0 - cb[2]));
      one_cell = clear > kOneCell;
      if (!(clear > 0.f)) {
        if (terrain_type >= 2 && tpar[0] < 0.5f * (fy1 - fy0)) ttop = terrain_top;
        else {
          float xs = fx0;
          bool open = true;             // the walk has not reached the footprint's high end yet
#pragma unroll 1
          for (int k = 0; k < 8 && open; ++k) {
            float wb[4];
            ttop = fmaxf(ttop, terrain_cell(terrain_type, tpar, xs, my, wb));
            ttop = fmaxf(ttop, fmaxf(terrain_height(terrain_type, tpar, xs, fy0), terrain_height(terrain_type, tpar, xs, fy1)));
            open = wb[1] <= fx1;
            xs = wb[1] + kProbeEps;
          }
          if (open) ttop = terrain_top; // more cells than the walk takes: no local bound
        }
      }
      g_ttop = ttop;
    }
    near = dc - bs_r - ttop <= g_margin;
    const float z0 = dot(n, p0) - pd, z1 = dot(n, p1) - pd;      // heights over the ground plane
    float d0 = z0 - rad, d1 = z1 - rad;
    // hulls: (p0, p1, rad) is the hull's bounding cylinder — a thin tarsal segment hovering inside its bounding sphere's
    // reach but above its own thickness needs no vertex scan
    // (capsules: its end spheres; over a terrain nothing above the highest top under the footprint needs a probe)
    if (g_type == GEOM_HULL) {
      // the cylinder's lowest point: the lower end disc's rim, rad * sin(axis, normal) below its centre (a steep tibia or
      // femur stays clear of the ground by far more than its end's height minus its radius says)
      const V3 ax = p1 - p0;
      const float ca = dot(n, ax);
      const float sn = sqrtf(fmaxf(0.f, 1.f - ca * ca / fmaxf(dot(ax, ax), 1e-12f)) + 4e-6f);
      near = near && fminf(z0, z1) - rad * fminf(sn, 1.f) - ttop <= g_margin;
    } else if (rough) near = near && fminf(d0, d1) - ttop <= g_margin;
    if (near && g_type == GEOM_CAPSULE) {
      float dw0 = kFar, dw1 = kFar; int w0 = 0, w1 = 0;
      if (rough) {
        if (one_cell && fminf(d0, d1) - g_ttop >= -kOneCell) { d0 -= g_ttop; d1 -= g_ttop; }      // what the probes would return
        else {
          terrain_probe(terrain_type, tpar, walls, p0.x, p0.y, z0, rad, g_margin, d0, dw0, w0);
          terrain_probe(terrain_type, tpar, walls, p1.x, p1.y, z1, rad, g_margin, d1, dw1, w1);
        }
      }
      const V3 q0 = ((p0 - rad * n) - (0.5f * d0) * n) - o, q1 = ((p1 - rad * n) - (0.5f * d1) * n) - o;
      if (d0 <= g_margin) { cd0 = d0; cp0 = q0; cnt = 1; }
      if (d1 <= g_margin) { if (cnt) { cd1 = d1; cp1 = q1; } else { cd0 = d1; cp0 = q1; } cnt++; }
      if (rough) {      // side faces: the end sphere's point towards the face, moved half the distance back
        if (w0 && dw0 <= g_margin) { const V3 nw = contact_frame(w0, Frame{n, n, n}).n; cdw0 = dw0; cpw0 = ((p0 - rad * nw) - (0.5f * dw0) * nw) - o; cfid = w0; cntw = 1; }
        if (w1 && dw1 <= g_margin) { const V3 nw = contact_frame(w1, Frame{n, n, n}).n; const V3 q = ((p1 - rad * nw) - (0.5f * dw1) * nw) - o;
                                     if (cntw) { cdw1 = dw1; cpw1 = q; cfid |= w1 << 3; } else { cdw0 = dw1; cpw0 = q; cfid = w1; } cntw++; }
        cnt += cntw;
      }
    }
  }
  SUB(21);
  // ---- phase 2: near convex hulls one after the other, each scanned by the whole wave; the geom's
  // parameters are broadcast from its lane's registers (no memory round trip)
  // (measured and dropped: holding a hull's vertices and distances in registers across the four scans, and handing the
  // few patch candidates over through LDS — same rate on flat ground, where the tarsal capsules make the contacts, and
  // 3-8 % slower over relief: six slots per lane whatever the hull's size, and 40 more callee-saved registers)
  unsigned long long hmask = __ballot(near && g_type == GEOM_HULL);
  const unsigned long long one_mask = __ballot(one_cell);
  SUB_COUNT(24, __popcll(hmask));
  while (hmask) {
    SUBH_T0();
    const int g = __ffsll((long long)hmask) - 1;
    hmask &= hmask - 1;
    const int b = __builtin_amdgcn_readlane(g_body, g);
    const float margin = readlane_f(g_margin, g);
    const gptr<float> V = hull_vert + 3 * __builtin_amdgcn_readlane(g_hadr, g);
    const int nvv = __builtin_amdgcn_readlane(g_hnum, g);
    const float* R = s.xmat()[b];
    const V3 xp = ld3(s.xpos()[b]);
    const V3 nb = matT_vec(R, n);
    const float c0 = dot(n, xp) - pd;
    // distance of a hull vertex to the ground under it (flat ground: the plane distance; terrains: the top of its cell, or
    // kFar when a side face owns the vertex — terrain_probe)
    // A hull inside one cell (above): every vertex is further than kOneCell from the cell's boundary, so terrain_probe
    // would return (height over the plane) - (the cell's top) and no face for each of them — as long as none is deeper
    // than kOneCell inside the box (then a way out sideways could be nearer than the top: checked after the first scan,
    // which is repeated with the probe if so).  Same values, without a probe per vertex.  Any other hull: a vertex more
    // than the margin above the highest top under the hull's footprint touches neither a top nor a face (a face looks
    // at it only from a higher cell) — it needs no probe either, and its height over that top, a lower bound of its
    // distance, keeps it out of every selection.
    float pdw = kFar; int pw_code = 0;          // side face of the vertex probed last
    bool one = rough && ((one_mask >> g) & 1ull);
    const float h_top = rough ? readlane_f(g_ttop, g) : 0.f;
    auto vdist = [&](V3 v) {
      float di = dot(nb, v) + c0;
      if (rough) {
        pw_code = 0;
        if (one || di - h_top > margin) di = di - h_top;
        else { const V3 pw = mat_vec(R, v) + xp; terrain_probe(terrain_type, tpar, walls, pw.x, pw.y, di, 0.f, margin, di, pdw, pw_code); }
      }
      return di;
    };
    // scan 1 — the deepest vertex — is all most near hulls ever get (a tarsal segment next to the one in contact: its
    // bounding cylinder reaches the margin, its vertices do not), and a plain loop pays one memory round trip per 64
    // vertices: the loads of four passes are issued together (indices clamped, results of the overhang ignored)
    SUBH(28);
    float best = INFINITY; int bi = 0x7fffffff;
    float bestw = INFINITY; int biw = 0x7fffffff;        // the vertex nearest to (deepest in) a side face: index * 8 + face code
    // (terrains: the vertices within the margin are compacted into a list on the way, in index order — the patch scans
    // then run over that list, lane = candidate)
    int ncand = 0;
    for (;;) {
    best = INFINITY; bi = 0x7fffffff; ncand = 0;
    for (int base = lane; base < nvv + lane; base += 4 * kWave) {
      V3 hv[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) { const int i = base + k * kWave; hv[k] = ld3(V + 3 * (i < nvv ? i : nvv - 1)); }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i = base + k * kWave;
        bool c = false; float di = 0.f;
        if (i < nvv) {
          di = vdist(hv[k]);
          if (di < best) { best = di; bi = i; }
          if (rough && pw_code && pdw < bestw) { bestw = pdw; biw = i * 8 + pw_code; }
          c = di <= margin;
        }
        if constexpr (kListed) {
          const unsigned long long cm = __ballot(c);
          const int pos = ncand + __popcll(cm & ((1ull << lane) - 1ull));
          if (c && pos < kCand) { cand_idx[pos] = i; cand_d[pos] = di; }
          ncand += __popcll(cm);
        }
      }
    }
    wave_argmin(best, bi);
    if (rough && one && !(best >= -kOneCell)) { one = false; continue; }
    break;
    }
    const float dmin = best; const int ia = bi;
    bool face = false;
    if (rough && walls) { wave_argmin(bestw, biw); face = bestw <= margin; }
    SUBH(29); SUB_COUNT(32, one ? 1 : 0); SUB_COUNT(33, nvv);
    if (!(dmin <= margin) && !face) { SUB_COUNT(25, 1); SUB_COUNT(26, (unsigned long long)(fminf(dmin, 1.f) * 1e6f)); continue; }
    SUB_COUNT(27, 1);
    int nsel = 0;
    int s1 = -1, s2 = -1, s3 = -1;
    [[maybe_unused]] int listed_dbg = 0;
    if (dmin <= margin) {
    nsel = 1;
    const float thr = fminf(dmin + hull_skin, margin);
    const V3 va = ld3(V + 3 * ia);
    bool listed = false;
    if constexpr (kListed) listed = ncand <= kCand;
    listed_dbg = listed ? 1 : 0;
    if (listed) {
      // terrains: the patch scans run over the listed vertices, lane = candidate — the same selections (same expressions,
      // lowest index among ties) without another pass over the hull's vertices, i.e. without three memory round trips
      // per scan and a terrain probe per vertex
      if constexpr (kListed) {
        WSYNC();
        const bool have = lane < ncand;
        const int ci = have ? cand_idx[lane] : 0;
        const bool ok = have && !(cand_d[have ? lane : 0] > thr);
        const V3 vi = ld3(V + 3 * ci);
        auto pick = [&](int idx) {      // coordinates of candidate vertex idx, from the lane that holds it
          const int wl = __ffsll((long long)__ballot(ok && ci == idx)) - 1;
          return v3(readlane_f(vi.x, wl), readlane_f(vi.y, wl), readlane_f(vi.z, wl));
        };
        { const V3 e = vi - va; best = ok ? dot(e, e) : -INFINITY; bi = ok ? ci : 0x7fffffff; }
        wave_argmax(best, bi);
        if (best > 1e-10f) {
          s1 = bi; nsel = 2;
          const V3 ab = pick(bi) - va;
          const float lab2 = dot(ab, ab);
          { const V3 cr = cross(vi - va, ab); best = ok ? dot(cr, cr) : -INFINITY; bi = ok ? ci : 0x7fffffff; }
          wave_argmax(best, bi);
          if (best > 1e-10f * lab2) {
            s2 = bi; nsel = 3;
            const float side = dot(cross(pick(bi) - va, ab), nb);
            const float sg = side > 0.f ? -1.f : 1.f;
            best = ok ? sg * dot(cross(vi - va, ab), nb) : -INFINITY; bi = ok ? ci : 0x7fffffff;
            wave_argmax(best, bi);
            if (best > sqrtf(1e-10f * lab2)) { s3 = bi; nsel = 4; }
          }
        }
        WSYNC();
      }
    } else {
    // b: farthest candidate from a
    best = -INFINITY; bi = 0x7fffffff;
    for (int i = lane; i < nvv; i += kWave) {
      V3 vi = ld3(V + 3 * i);
      float di = vdist(vi);
      if (di > thr) continue;
      V3 e = vi - va; float sc = dot(e, e);
      if (sc > best) { best = sc; bi = i; }
    }
    wave_argmax(best, bi);
    if (best > 1e-10f) {
      s1 = bi; nsel = 2;
      const V3 ab = ld3(V + 3 * bi) - va;
      const float lab2 = dot(ab, ab);
      best = -INFINITY; bi = 0x7fffffff;
      for (int i = lane; i < nvv; i += kWave) {
        V3 vi = ld3(V + 3 * i);
        float di = vdist(vi);
        if (di > thr) continue;
        V3 cr = cross(vi - va, ab); float sc = dot(cr, cr);
        if (sc > best) { best = sc; bi = i; }
      }
      wave_argmax(best, bi);
      if (best > 1e-10f * lab2) {
        s2 = bi; nsel = 3;
        const float side = dot(cross(ld3(V + 3 * bi) - va, ab), nb);
        const float sg = side > 0.f ? -1.f : 1.f;
        best = -INFINITY; bi = 0x7fffffff;
        for (int i = lane; i < nvv; i += kWave) {
          V3 vi = ld3(V + 3 * i);
          float di = vdist(vi);
          if (di > thr) continue;
          float sc = sg * dot(cross(vi - va, ab), nb);
          if (sc > best) { best = sc; bi = i; }
        }
        wave_argmax(best, bi);
        if (best > sqrtf(1e-10f * lab2)) { s3 = bi; nsel = 4; }
      }
    }
    }
    nsel = nsel < max_hull_contacts ? nsel : max_hull_contacts;
    }   // a vertex within the margin of the top of its cell
    SUBH(30); SUB_COUNT(34, listed_dbg);
    if (lane < nsel && nh + lane < kMaxCon) {
      const int vi = lane == 0 ? ia : lane == 1 ? s1 : lane == 2 ? s2 : s3;
      const V3 v = ld3(V + 3 * vi);
      // The deepest vertex keeps the distance the scan found for it.  Over a terrain a second evaluation is not guaranteed to
      // agree with the scan's: a vertex within rounding of a cell boundary can be a top contact for one inlined copy of the
      // probe and a side face's (top distance kFar) for the other — round 3 stored that kFar as the contact's distance, a
      // contact 1e30 mm away that the solver then carried as a row.  The other patch vertices were selected with a distance
      // <= thr: one that comes back larger is the same tie and is stored at thr.
      float dist = lane == 0 ? dmin : vdist(v);
      if (rough && lane != 0 && !(dist <= margin)) dist = fminf(dmin + hull_skin, margin);
      const V3 pw = mat_vec(R, v) + xp;
      X.info[nh + lane] = (g0 + g) | (lane << 8) | (b << 12);
      X.dist[nh + lane] = dist;
      st3(X.r[nh + lane], (pw - (0.5f * dist) * n) - o);
    }
    if (face && lane == nsel && nh + lane < kMaxCon) {      // the side-face contact of this hull: its own frame
      const int code = biw & 7;
      const V3 nw = contact_frame(code, Frame{n, n, n}).n;
      const V3 pw = mat_vec(R, ld3(V + 3 * (biw >> 3))) + xp;
      X.info[nh + lane] = (g0 + g) | (lane << 8) | (b << 12) | (code << 20);
      X.dist[nh + lane] = bestw;
      st3(X.r[nh + lane], (pw - (0.5f * bestw) * nw) - o);
    }
    nsel += face ? 1 : 0;
    if (lane == g) cnt = nsel;
    nh += nsel;
    SUBH(31);
  }
  SUB(22);
  // ---- phase 3: contact slots in geom order.  cnt <= 4, so an exclusive prefix over lanes is three ballots.
  const unsigned long long b0 = __ballot(cnt & 1), b1 = __ballot(cnt & 2), b2 = __ballot(cnt & 4);
  const unsigned long long lt = (1ull << lane) - 1ull;
  const int slot0 = __popcll(b0 & lt) + 2 * __popcll(b1 & lt) + 4 * __popcll(b2 & lt);
  const int sl = slot_base + slot0;
  geom_slot0[gi] = slot_base + slot0;
  if (g_type == GEOM_CAPSULE && cnt > 0) {
    const int ntop = cnt - cntw;       // top (ground-plane frame) contacts first, then the side faces
    if (ntop > 0 && sl < kMaxCon) { s.c_info[sl] = info_pack(gi, -1, g_body, 0); s.c_D[sl] = cd0; st3(s.c_r[sl], cp0); }
    if (ntop > 1 && sl + 1 < kMaxCon) { s.c_info[sl + 1] = info_pack(gi, -1, g_body, 0); s.c_D[sl + 1] = cd1; st3(s.c_r[sl + 1], cp1); }
    if (cntw > 0 && sl + ntop < kMaxCon) { s.c_info[sl + ntop] = info_pack(gi, -1, g_body, 0) | ((cfid & 7) << 24); s.c_D[sl + ntop] = cdw0; st3(s.c_r[sl + ntop], cpw0); }
    if (cntw > 1 && sl + ntop + 1 < kMaxCon) { s.c_info[sl + ntop + 1] = info_pack(gi, -1, g_body, 0) | ((cfid >> 3) << 24); s.c_D[sl + ntop + 1] = cdw1; st3(s.c_r[sl + ntop + 1], cpw1); }
  }
  slot_base += __popcll(b0) + 2 * __popcll(b1) + 4 * __popcll(b2);
  }   // passes of 64 geoms
  const int total = slot_base;
  WSYNC();
  if (lane < nh && lane < kMaxCon) {
    const int info = X.info[lane];
    const int slot = geom_slot0[info & 0xff] + ((info >> 8) & 0xf);
    if (slot < kMaxCon) { s.c_info[slot] = info_pack(info & 0xff, -1, (info >> 12) & 0xff, 0) | (((info >> 20) & 7) << 24); s.c_D[slot] = X.dist[lane]; st3(s.c_r[slot], ld3(X.r[lane])); }
  }
  const int cap = m.max_contacts;      // <= kMaxCon (nmf_batch_set_contact_capacity)
  const int ncon = total > cap ? cap : total;
  if (lane == 0) { s.ncon = ncon; s.overflow = total > cap ? 1 : 0; }
  WSYNC();
  {   // contacts with a terrain side face (their own frames): the stages that follow take the general path only if there are any
    if constexpr (rough) {
      const unsigned long long wf = __ballot(lane < ncon && info_fid(s.c_info[lane]) != 0);
      if (lane == 0) s.nwall = __popcll(wf);
    }
  }
  // body_cstart[b] = number of contacts on bodies before b = the first contact of a body >= b (the list is in geom order,
  // geoms in body order).  Skeletons of up to 63 bodies: lane c marks where a body's range starts, lane 63 - b takes a
  // prefix minimum over the starts of the bodies from b on — two LDS round trips and six DPP steps, where a count over
  // the whole list per body was a dependent LDS read per contact (round 5: a sixth of this stage's cycles on flat ground,
  // more on the blocks' 7.4 contacts).
  bool ranged = false;
  if constexpr (TP::kStar) { if constexpr (TP::NB + 1 <= kWave) {
    ranged = true;
    const int e = lane < ncon ? info_body(s.c_info[lane]) : 0x7fffffff;
    const int e_prev = lane > 0 && lane - 1 < ncon ? info_body(s.c_info[lane > 0 ? lane - 1 : 0]) : -1;
    if (lane <= TP::NB) s.body_cstart[lane] = (typename FlyLds<TP>::cstart_t)ncon;
    WSYNC();
    if (lane < ncon && e != e_prev) s.body_cstart[e] = (typename FlyLds<TP>::cstart_t)lane;
    WSYNC();
    const int b = kWave - 1 - lane;
    const int first = wave_prefix_min_int(b <= TP::NB ? (int)s.body_cstart[b <= TP::NB ? b : 0] : 0x7fffffff);
    WSYNC();
    if (b <= TP::NB) s.body_cstart[b] = (typename FlyLds<TP>::cstart_t)first;
  } }
  if (!ranged) {
    for (int b = lane; b <= s.nb(); b += kWave) {
      int c_before = 0;
      for (int c = 0; c < ncon; ++c) c_before += info_body(s.c_info[c]) < b ? 1 : 0;
      s.body_cstart[b] = (typename FlyLds<TP>::cstart_t)c_before;
    }
  }
  WSYNC();
  SUB(23);
}

// ------------------------------------------------------------------ chain sweeps
// Lane layout for everything that walks a leg: the wave is 8 groups of 8 lanes; group g < NLEG owns
// leg g and lane r < 6 of the group owns component r of a spatial vector (or row r of a 6x6).
// Groups >= NLEG shadow the last leg and lanes r >= 6 shadow row 5: they compute bit-identical values and
// store them to the same LDS words as their twins, so the sweeps are branch-free straight-line code (no exec
// masking) and the DPP reductions stay converged; `mask` removes the shadow rows from group sums.
// T[b] = twist of body b under generalized vector x:  T_b = T_parent + sum_j S_j x_j
// hybrid kernels: true while the Newton loop runs on the reduced problem (root + legs; see physics_forward)
template <class TP>
__device__ __forceinline__ bool rest_reduced(const FlyLds<TP>& s) {
  if constexpr (TP::kStar) { if constexpr (TP::REST_B > 0) return __builtin_amdgcn_readfirstlane(s.reduced) != 0; }
  return false;
}
// Lane-strided loops over the dofs / bodies a stage has to visit: all of them — or, on the hybrid kernels while the Newton
// loop runs on the reduced problem, root + legs only, compacted: 72 of ALL_BIOLOGICAL's 132 dofs are two passes of the wave
// instead of three (the third for four dofs), its 49 of 69 bodies one pass instead of two.
template <class TP, class F>
__device__ __forceinline__ void for_dofs(const FlyLds<TP>& s, bool red, int lane, F&& f) {
  if constexpr (TP::kStar) { if constexpr (TP::REST_V > 0) {
    if (red) { for (int jj = lane; jj < TP::NV - TP::REST_V; jj += kWave) f(jj < 6 ? jj : jj + TP::REST_V); return; }
  } }
  for (int j = lane; j < s.nv(); j += kWave) f(j);
}
template <class TP, class F>
__device__ __forceinline__ void for_bodies(const FlyLds<TP>& s, bool red, int lane, F&& f) {
  if constexpr (TP::kStar) { if constexpr (TP::REST_B > 0) {
    if (red) { for (int bb = lane; bb < TP::NB - TP::REST_B; bb += kWave) f(bb < 1 ? 0 : bb + TP::REST_B); return; }
  } }
  for (int b = lane; b < s.nb(); b += kWave) f(b);
}

// restA * t  (the rest's articulated inertia applied to the root twist)
template <class TP>
__device__ __forceinline__ SV rest_inertia_mul(const FlyLds<TP>& s, SV t) {
  const float tv[6] = {t.a.x, t.a.y, t.a.z, t.l.x, t.l.y, t.l.z};
  float o[6];
#pragma unroll
  for (int r = 0; r < 6; r++) {
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < 6; c++) {
      const int i = r < c ? r : c, jx = r < c ? c : r;
      acc += s.restA[i * 6 - i * (i - 1) / 2 + (jx - i)] * tv[c];
    }
    o[r] = acc;
  }
  return SV{v3(o[0], o[1], o[2]), v3(o[3], o[4], o[5])};
}

template <class TP>
__device__ void sweep_twists(FlyLds<TP>& s, const float* x, float (*T)[row_width_tw<TP>()], const GModel& m, int lane) {
  if constexpr (!TP::kStar) { tree_sweep_twists(s, x, T, m, lane); return; } else {
  const LaneRole L = lane_role<TP>(lane);
  float t = 0.f;
#pragma unroll
  for (int j = 0; j < 6; ++j) t += x[j] * s.S[j][L.rr];
  if (lane < 6) T[0][lane] = t;
  const int j0 = TP::LD0 + L.lg * TP::NDL, b0 = TP::LB0 + L.lg * TP::NBL;
  float px[TP::NDL];      // (the chain's inputs first: see the velocity stage)
#pragma unroll
  for (int d = 0; d < TP::NDL; ++d) px[d] = x[j0 + d] * s.S[j0 + d][L.rr];
  static_for<TP::NDL>([&](auto D) {
    constexpr int d = decltype(D)::value;
    t += px[d];
    if constexpr (TP::is_last(d)) T[b0 + TP::lbody(d)][L.rr] = t;
  });
  WSYNC();
  if constexpr (TP::REST_B > 0) { if (!rest_reduced(s)) tree_sweep_twists_levels(s, x, T, m, lane); }
  }
}

// W[b] <- sum of W over the subtree of b (in place), then emit(j, S_j · W[body(j)]) for every dof j
// (the projection and whatever the caller does with it share one pass: no intermediate vector, no extra sync)
template <class TP, class Emit>
__device__ __forceinline__ void sweep_project(FlyLds<TP>& s, float (*W)[row_width_tw<TP>()], const GModel& m, int lane, Emit&& emit) {
  if constexpr (!TP::kStar) { tree_sweep_project(s, W, m, lane, [](int, SV w) { return w; }, emit); return; } else {
  const bool red = rest_reduced(s);
  if constexpr (TP::REST_B > 0) { if (!red) tree_gather_levels(s, W, m, lane, [](int, SV w) { return w; }); }
  const LaneRole L = lane_role<TP>(lane);
  const int b0 = TP::LB0 + L.lg * TP::NBL;
  float acc = 0.f;
  {
    float pw[TP::NBL];
#pragma unroll
    for (int l = 0; l < TP::NBL; ++l) pw[l] = W[b0 + l][L.rr];
    static_for<TP::NBL>([&](auto I) {
      constexpr int l = TP::NBL - 1 - decltype(I)::value;
      acc += pw[l];
      W[b0 + l][L.rr] = acc;
    });
  }
  // root = own + the six leg bases (group sums are free: every group holds its base in acc)
  WSYNC();
  if (lane < 6) {
    float a0 = W[0][lane];
#pragma unroll
    for (int k = 0; k < TP::NLEG; ++k) a0 += W[TP::LB0 + k * TP::NBL][lane];
    if constexpr (TP::REST_B > 0) {
      if (!red) for (int k = (int)s.t_cstart[0]; k < (int)s.t_cstart[0] + (int)s.t_ccount[0]; ++k) a0 += W[(int)s.t_body[k]][lane];
    }
    W[0][lane] = a0;
  }
  WSYNC();
  if constexpr (TP::REST_V == 0 && TP::NV > kWave && TP::NV <= 2 * kWave) {
    // (leg-chain kernels: both turns' products before the first turn's emit — emit stores, see the velocity stage's pass 2)
    const int jb = lane + kWave;
    const bool two = jb < TP::NV;
    const float pa = dot(ldsv(s.S[lane]), ldsv(W[dof_body_of<TP>(lane)]));
    float pb = 0.f;
    if (two) pb = dot(ldsv(s.S[jb]), ldsv(W[dof_body_of<TP>(jb)]));
    emit(lane, pa);
    if (two) emit(jb, pb);
  } else {
    for_dofs(s, red, lane, [&](int j) {         // reduced problem: the rest's dofs are not in it
      emit(j, dot(ldsv(s.S[j]), ldsv(W[j >= TP::LD0 || j < 6 ? dof_body_of<TP>(j) : tbl_dofbody(s, j)])));
    });
  }
  WSYNC();
  }
}

// y = M x  (composite-free inverse dynamics with zero velocity / gravity); leaves T = twists(x).
// have_twists: T already holds twists(x) (the ABA leaves them there).
template <class TP, class Emit>
__device__ __forceinline__ void mul_M(FlyLds<TP>& s, const float* x, const GModel& m, int lane, bool have_twists, Emit&& emit) {
  if (!have_twists) sweep_twists(s, x, s.T, m, lane);
  const bool red = rest_reduced(s);
  for_bodies(s, red, lane, [&](int b) {
    const SV tb = ldsv(s.T[b]);
    SV wb = inert_mul(s.Ib[b], tb);
    if constexpr (TP::kStar) { if constexpr (TP::REST_B > 0) { if (red && b == 0) wb = wb + rest_inertia_mul(s, tb); } }
    stsv(s.W[b], wb);
  });
  WSYNC();
  sweep_project(s, s.W, m, lane, [&](int j, float v) { emit(j, v + s.arm[j] * x[j]); });
}

// Row r of the 6x6 spatial inertia [[I, [h]x], [-[h]x, m 1]] read straight out of the 10-float form (m, hx, hy, hz,
// Ixx, Iyy, Izz, Ixy, Ixz, Iyz): entry c = sgn[r][c] * I10[idx[r][c]].  A second, 21-float copy of every body's inertia
// (4 KB of LDS) bought nothing but the row fetch; with the map a row costs the same six LDS reads and six fused
// multiply-adds into the articulated inertia.
constexpr int kInertiaIdx[6][6] = {{4, 7, 8, 0, 3, 2}, {7, 5, 9, 3, 0, 1}, {8, 9, 6, 2, 1, 0},
                                   {0, 3, 2, 0, 0, 0}, {3, 0, 1, 0, 0, 0}, {2, 1, 0, 0, 0, 0}};
constexpr int kInertiaSgn[6][6] = {{1, 1, 1, 0, -1, 1}, {1, 1, 1, 1, 0, -1}, {1, 1, 1, -1, 1, 0},
                                   {0, 1, -1, 1, 0, 0}, {-1, 0, 1, 0, 1, 0}, {1, -1, 0, 0, 0, 1}};
struct InertiaRowMap { int off[6]; float sg[6]; };      // byte offsets into a body's Ib row, signs (+1, -1, 0)
// packed per row index for the launch's table (k_tab[r][11..13]): byte offsets of columns 0-2, of columns 3-5, (sign + 1) x 2 bits
__device__ __forceinline__ void inertia_map_pack(int r, int* words) {
  int wa = 0, wb = 0, wc = 0;
  static_for<6>([&](auto R) {
    constexpr int rr = decltype(R)::value;
    constexpr int a = 4 * (kInertiaIdx[rr][0] | kInertiaIdx[rr][1] << 8 | kInertiaIdx[rr][2] << 16);
    constexpr int b = 4 * (kInertiaIdx[rr][3] | kInertiaIdx[rr][4] << 8 | kInertiaIdx[rr][5] << 16);
    constexpr int c = (kInertiaSgn[rr][0] + 1) | (kInertiaSgn[rr][1] + 1) << 2 | (kInertiaSgn[rr][2] + 1) << 4 |
                      (kInertiaSgn[rr][3] + 1) << 6 | (kInertiaSgn[rr][4] + 1) << 8 | (kInertiaSgn[rr][5] + 1) << 10;
    if (r == rr) { wa = a; wb = b; wc = c; }
  });
  words[0] = wa; words[1] = wb; words[2] = wc;
}
__device__ __forceinline__ InertiaRowMap inertia_map_unpack(const float* q) {
  const int wa = __float_as_int(q[11]), wb = __float_as_int(q[12]), wc = __float_as_int(q[13]);
  InertiaRowMap M;
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    M.off[c] = ((c < 3 ? wa : wb) >> (8 * (c % 3))) & 0xff;
    M.sg[c] = (float)((wc >> (2 * c)) & 3) - 1.f;
  }
  return M;
}
// IA += row r of body b's spatial inertia
template <class TP>
__device__ __forceinline__ void add_inertia_row(float* IA, const FlyLds<TP>& s, int b, const InertiaRowMap& M) {
  const char* base = reinterpret_cast<const char*>(&s.Ib[b][0]);
  float v[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) v[c] = *reinterpret_cast<const float*>(base + M.off[c]);
#pragma unroll
  for (int i = 0; i < 3; ++i) {       // packed: sign pair x value pair + row pair
    const f2 r = __builtin_elementwise_fma(mk2(M.sg[2 * i], M.sg[2 * i + 1]), mk2(v[2 * i], v[2 * i + 1]), mk2(IA[2 * i], IA[2 * i + 1]));
    IA[2 * i] = r.x; IA[2 * i + 1] = r.y;
  }
}

// row `r` of the contact stiffness  K_c = D * sum_{active rows k} l_k l_kT,  l_k = l_n +/- mu l_t,  l_m = (rc x d_m ; d_m)
// for the frame directions d_m = n, t1, t2.  With M3 the symmetric 3x3 of pyramid coefficients over (n, t1, t2) — D sum a,
// D mu (a0 - a1), D mu (a2 - a3), D mu^2 (a0 + a1), D mu^2 (a2 + a3) — and o_m = l_m[r] the lane's own components,
//   row = sum_m C_m l_m = (rc x w ; w),   C = M3 o,   w = sum_m C_m d_m :
// the cross product is taken once, of the combined direction, instead of three times.
// KLane: what depends on the lane's row index and the (wave-uniform) contact frame only.
struct KLane { float dA[3], dB[3], dO[3]; int ia, ib; };
__device__ __forceinline__ KLane k_lane(int r, const Frame& fr) {
  KLane K;
  const bool top = r < 3;
  const int k = top ? r : r - 3;
  K.ia = k == 2 ? 0 : k + 1; K.ib = k == 0 ? 2 : k - 1;       // (rc x d)[k] = rc[ia] d[ib] - rc[ib] d[ia]
  const V3 d[3] = {fr.n, fr.t1, fr.t2};
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    const float da = K.ib == 0 ? d[m].x : (K.ib == 1 ? d[m].y : d[m].z), db = K.ia == 0 ? d[m].x : (K.ia == 1 ? d[m].y : d[m].z);
    const float dk = k == 0 ? d[m].x : (k == 1 ? d[m].y : d[m].z);
    K.dA[m] = top ? da : 0.f; K.dB[m] = top ? db : 0.f; K.dO[m] = top ? 0.f : dk;
  }
  return K;
}
// `walls` (terrain kernels only): some contact of this step touches a terrain side face — the contact's frame id decides,
// and a face's row constants are built on the spot (wave-uniform flag: face-free steps never look)
template <class TP>
__device__ __forceinline__ void add_contact_K_row(float* row, const FlyLds<TP>& s, int c, const KLane& K0, const Frame& fr0, int r = 0,
                                                  bool walls = false) {
  KLane K = K0; Frame fr = fr0;
  if constexpr (TP::kTerrain) {
    if (walls) {
      const int fid = info_fid(s.c_info[c]);
      if (fid) { fr = contact_frame(fid, fr0); K = k_lane(r, fr); }
    }
  }
  float m_nn, m_n1, m_n2, m_11, m_22;
  if constexpr (kHasCm3<TP>) {
    const float* q = s.c_m3[c];
    m_nn = q[0]; m_n1 = q[1]; m_n2 = q[2]; m_11 = q[3]; m_22 = q[4];
    if (m_nn == 0.f) return;                       // no active row
  } else {
    const int act = info_act(s.c_info[c]);
    if (!act) return;
    const float D = s.c_D[c], mu = s.c_mu[c];
    const float a0 = (act & 1) ? 1.f : 0.f, a1 = (act & 2) ? 1.f : 0.f, a2 = (act & 4) ? 1.f : 0.f, a3 = (act & 8) ? 1.f : 0.f;
    const float Dm = D * mu, Dmm = Dm * mu;
    m_nn = D * (a0 + a1 + a2 + a3); m_n1 = Dm * (a0 - a1); m_n2 = Dm * (a2 - a3); m_11 = Dmm * (a0 + a1); m_22 = Dmm * (a2 + a3);
  }
  const V3 rc = ld3(s.c_r[c]);
  const float rcA = s.c_r[c][K.ia], rcB = s.c_r[c][K.ib];
  const float o_n = fmaf(rcA, K.dA[0], fmaf(-rcB, K.dB[0], K.dO[0]));
  const float o_1 = fmaf(rcA, K.dA[1], fmaf(-rcB, K.dB[1], K.dO[1]));
  const float o_2 = fmaf(rcA, K.dA[2], fmaf(-rcB, K.dB[2], K.dO[2]));
  const float C_n = m_nn * o_n + m_n1 * o_1 + m_n2 * o_2, C_1 = m_n1 * o_n + m_11 * o_1, C_2 = m_n2 * o_n + m_22 * o_2;
  const V3 w = C_n * fr.n + C_1 * fr.t1 + C_2 * fr.t2;
  const V3 x = cross(rc, w);
  row[0] += x.x; row[1] += x.y; row[2] += x.z; row[3] += w.x; row[4] += w.y; row[5] += w.z;
}

// Articulated-body solve of (CRBA(I_b [+ K_b]) + diag(delta)) x = tau, delta_j = armature_j +
// hdamp * damping_j (root dofs carry no armature/damping).  Leaves T = twists(x).
//   backward sweep : per leg, rows of the articulated inertia IA and of the bias wrench pA are
//                    spread over the 6 lanes of the leg's group; per hinge: U = IA s, D = s.U + delta,
//                    IA -= U UT / D, pA += U (tau - s.pA) / D   (group sums by DPP)
//   root           : IA_root a = (wrench of tau_root) - pA_root, 6x6 Cholesky in one lane
//   forward sweep  : x_j = (u_j - U_j . a) / D_j,  a += s_j x_j
// one articulated-body elimination step for hinge/axis `sj` (6 floats, group-uniform) with this lane's row IA,
// bias component pA, own component `sown`, diagonal term delta and generalized force tauj
__device__ __forceinline__ void aba_step(float (&IA)[6], float& pA, const float* sj, float sown, float mask, float delta,
                                         float tauj, float& Uout, float& uout, float& invDout) {
  // row arithmetic in packed float32, as in aba_step_scaled below
  f2 acc = mk2(IA[0], IA[1]) * mk2(sj[0], sj[1]);
  acc = __builtin_elementwise_fma(mk2(IA[2], IA[3]), mk2(sj[2], sj[3]), acc);
  acc = __builtin_elementwise_fma(mk2(IA[4], IA[5]), mk2(sj[4], sj[5]), acc);
  const float U = acc.x + acc.y;
  const float sr = mask * sown;
  const float D = grp8_sum(sr * U) + delta;
  const float sp = grp8_sum(sr * pA);
  const float invD = __builtin_amdgcn_rcpf(D);
  const float u = tauj - sp;
  const float k = U * invD;
  { const float bb[6] = {grp8_bcast<0>(U), grp8_bcast<1>(U), grp8_bcast<2>(U), grp8_bcast<3>(U), grp8_bcast<4>(U), grp8_bcast<5>(U)};
    fma6(IA, -k, bb); }
  pA += k * u;
  Uout = mask * U; uout = u; invDout = invD;
}
// the same for the leg chains of the star sweeps, whose back-substitution needs (u - U.a) / D only: hands back U / D and
// u / D (one register per dof less to keep, one multiply per dof less in the forward sweep).  `sr` is the lane's own axis
// component with the shadow rows already zero.  SHADOW0: the forward sweep keeps its accelerations zero in the shadow
// rows, so U / D needs no mask either.
template <bool SHADOW0>
__device__ __forceinline__ void aba_step_scaled(float (&IA)[6], float& pA, const float* sj, float sr, float mask, float delta,
                                                float tauj, float& UDout, float& uDout, float& Uraw, float& invDraw) {
  f2 a01 = mk2(IA[0], IA[1]), a23 = mk2(IA[2], IA[3]), a45 = mk2(IA[4], IA[5]);
  f2 acc = a01 * mk2(sj[0], sj[1]);
  acc = __builtin_elementwise_fma(a23, mk2(sj[2], sj[3]), acc);
  acc = __builtin_elementwise_fma(a45, mk2(sj[4], sj[5]), acc);
  const float U = acc.x + acc.y;
  const float D = grp8_sum(sr * U) + delta;
  const float sp = grp8_sum(sr * pA);
  const float invD = __builtin_amdgcn_rcpf(D);
  const float u = tauj - sp;
  const float k = U * invD;
  const f2 nk = mk2(-k, -k);
  a01 = __builtin_elementwise_fma(nk, mk2(grp8_bcast<0>(U), grp8_bcast<1>(U)), a01);
  a23 = __builtin_elementwise_fma(nk, mk2(grp8_bcast<2>(U), grp8_bcast<3>(U)), a23);
  a45 = __builtin_elementwise_fma(nk, mk2(grp8_bcast<4>(U), grp8_bcast<5>(U)), a45);
  IA[0] = a01.x; IA[1] = a01.y; IA[2] = a23.x; IA[3] = a23.y; IA[4] = a45.x; IA[5] = a45.y;
  pA += k * u;
  UDout = SHADOW0 ? k : mask * k; uDout = u * invD;
  Uraw = U; invDraw = invD;
}
// LDS pointer whose value the optimizer may not look through: the accesses made from it carry their (small, constant)
// offsets in the instruction — a ds_read2 reaches 255 dwords — instead of one address add per access pair, which is what
// `big constant array offset + lane-dependent row` turns into
typedef const __attribute__((address_space(3))) float* lds_cptr;
template <class T>
__device__ __forceinline__ lds_cptr lds_pinned(const T* p) {
  lds_cptr q = (lds_cptr)(const void*)p;
  asm("" : "+v"(q));
  return q;
}

// Where the contact-space solve (nmf_dual.h) keeps its data — all overlays of buffers that are dead between the smooth
// solve and the end of the constraint solve.  Per leg hinge / root axis a factor row of 8 floats: U / sqrt(D) (6),
// 1 / sqrt(D), pad; the root's six axes in elimination order (angular z, y, x, linear z, y, x).
//   kDualS: factors on c_w + c_m3, the rows' reference accelerations and later the hinge sums on vB;
//   kDualH: leg factors on vA..vD, the root's + reference accelerations + hinge sums on c_w (its rest hand-off slots are
//           consumed before the root is eliminated).
template <class TP> __device__ __forceinline__ float (*dual_leg(FlyLds<TP>& s))[8] {
  if constexpr (kDualGlob<TP>) return reinterpret_cast<float(*)[8]>(s.dual_glob[0]);      // HBM (generic pointer: callers go through gptr)
  else if constexpr (kDualH<TP>) {
    static_assert(!kDualH<TP> || kDualGlob<TP> || 4 * TP::NV >= TP::NLEG * TP::NDL * 8, "leg factors do not fit vA..vD");
    return reinterpret_cast<float(*)[8]>(&s.vA[0]);
  } else {
    static_assert(sizeof(float) * 8 * (TP::NLEG * TP::NDL + 6) <= sizeof(float) * 12 * kMaxCon, "articulated-body factors do not fit c_w + c_m3");
    return reinterpret_cast<float(*)[8]>(&s.c_w[0][0]);
  }
}
template <class TP> __device__ __forceinline__ float (*dual_root(FlyLds<TP>& s))[8] {
  if constexpr (kDualH<TP>) return reinterpret_cast<float(*)[8]>(&s.c_w[0][0]);
  else return dual_leg(s) + TP::NLEG * TP::NDL;
}
template <class TP> __device__ __forceinline__ float* dual_aref(FlyLds<TP>& s) {
  if constexpr (kDualH<TP>) return &s.c_w[0][0] + 48; else return s.vB;
}
// the contact wrenches Euler's solve applies as body forces: c_w, except in the hybrid kernels, whose solves use c_w for
// the rest's hand-off slots — physics_integrate copies them to vC first
template <class TP> __device__ __forceinline__ float (*dual_wrench(FlyLds<TP>& s))[7] {
  if constexpr (kDualH<TP>) {
    static_assert(!kDualH<TP> || 7 * kDualMaxCon<TP> <= TP::NV, "contact wrenches do not fit vC");
    return reinterpret_cast<float(*)[7]>(&s.vC[0]);
  } else return s.c_w;
}
template <class TP> __device__ __forceinline__ float* dual_acc(FlyLds<TP>& s) {       // [NLEG * NDL leg hinges | 6 root axes]
  if constexpr (kDualH<TP>) {
    static_assert(!kDualH<TP> || 96 + TP::NLEG * TP::NDL + 6 <= 7 * kMaxCon, "hinge sums do not fit c_w");
    return &s.c_w[0][0] + 96;
  } else {
    static_assert(TP::NLEG * TP::NDL + 6 <= 3 * TP::NV, "hinge sums do not fit vB..vD");
    return s.vB;
  }
}

// WITHK_ (leg-chain kernels that have the contact-space solve): the contact stiffness rows are compiled into the solve at all
// — only the primal Newton loop's instantiation has them, so the two solves of an ordinary step (smooth, Euler) run a function
// two thirds the size: the step's hot path has to share a 64 KB instruction cache.  Elsewhere one instantiation serves all.
template <class TP, bool WELD, bool WITHK_ = true>
__device__ __noinline__ void aba_solve(FlyLds<TP>& s, int tau_id, int x_id, bool withK, float hdamp,
                          const GModel& m, int lane, bool store = false, bool withF = false) {
  if constexpr (!TP::kStar) { tree_aba_solve<TP, WELD>(s, tau_id, x_id, withK, hdamp, m, lane); return; } else {
  withK = WITHK_ && __builtin_amdgcn_readfirstlane((int)withK) != 0;          // wave-uniform: scalar branches, no exec masking
  // store: keep the factors (U / sqrt D, 1 / sqrt D per hinge and root axis) in LDS for the contact-space solve (nmf_dual.h)
  store = kDual<TP> && __builtin_amdgcn_readfirstlane((int)store) != 0;
  // withF: the contact wrenches in c_w act on their bodies as external forces (the Euler step's solve after a contact-space
  // constraint solve: J^T f is never projected onto the dofs)
  withF = kDual<TP> && __builtin_amdgcn_readfirstlane((int)withF) != 0;
  const float* tau = s.vec(tau_id);
  float* x = s.vec(x_id);
  Frame fr{};
  if (withK) fr = ld_frame(s, m);
  const bool walls = TP::kTerrain && withK && __builtin_amdgcn_readfirstlane(s.nwall) != 0;      // terrain side faces in contact this step
  const LaneRole L = lane_role<TP>(lane);
  const int j0 = TP::LD0 + L.lg * TP::NDL, b0 = TP::LB0 + L.lg * TP::NBL;
  static_assert(sizeof(AbaHandoff<TP>) <= sizeof(float) * TP::NB * 12, "ABA hand-off does not fit T..W");
  AbaHandoff<TP>& H = *reinterpret_cast<AbaHandoff<TP>*>(&s.T[0][0]);
  // offsets of row rr inside a symmetric 6x6's packed storage (lane constants; the hybrid kernels' hand-off slots)
  int so[6];
#pragma unroll
  for (int c = 0; c < 6; c++) {
    if constexpr (kHasIsym<TP>) so[c] = __float_as_int(s.k_tab[L.rr][14 + c]);
    else { const int i = L.rr < c ? L.rr : c, jx = L.rr < c ? c : L.rr; so[c] = i * 6 - i * (i - 1) / 2 + (jx - i); }
  }
  InertiaRowMap IM{};                                              // this lane's row of a body's 6x6 inertia, read out of Ib
  if constexpr (!kHasIsym<TP>) IM = inertia_map_unpack(s.k_tab[L.rr]);
  // this lane's row of U_j, S_j; group-uniform u_j, 1/D_j.  Long chains (ALL_POSSIBLE: 24 dofs per leg) re-read S_j in the
  // forward sweep instead of keeping it: 24 registers fewer to spill
  constexpr bool kKeepS = TP::NDL <= 16;
  float Ureg[TP::NDL], ureg[TP::NDL], Sreg[kKeepS ? TP::NDL : 1];        // U / D (this lane's row), u / D, own axis component
  // Shadow rows (r = 6, 7).  Where S and T have a padding column (S's is zeroed at launch) they read their axis
  // component from it and keep the acceleration sweep's value there: zero contributions to every group sum without a
  // mask multiply per dof.  Without padding they shadow row 5 and the sums are masked.
  constexpr bool kShadow0 = row_width_s<TP>() > 6 && row_width_tw<TP>() > 6;
  const int rS = kShadow0 && L.r >= 6 ? 6 : L.rr;
  const lds_cptr Sleg = lds_pinned(&s.S[j0][0]), Sown = lds_pinned(&s.S[j0][rS]);
  constexpr int SW = row_width_s<TP>();
  KLane KL;                             // contact stiffness rows: per-row constants from the launch's table
  if (withK) {
    const float* q = s.k_tab[L.rr];
#pragma unroll
    for (int i = 0; i < 3; ++i) { KL.dA[i] = q[i]; KL.dB[i] = q[3 + i]; KL.dO[i] = q[6 + i]; }
    KL.ia = __float_as_int(q[9]); KL.ib = __float_as_int(q[10]);
  }
  int cs[TP::NBL + 1], cs_root0 = 0, cs_root1 = 0;                         // contact ranges of the leg's bodies / the root
  static_for<TP::NBL + 1>([&](auto I) { constexpr int l = decltype(I)::value; cs[l] = withK || withF ? s.body_cstart[b0 + l] : 0; });
  if (withK || withF) { cs_root0 = s.body_cstart[0]; cs_root1 = s.body_cstart[1]; }
  // hybrid: the rest of the body (head, abdomen, wings, ...) is eliminated level by level first; its children-of-root
  // hand their articulated inertias to the root below through s.slot
  const bool red = rest_reduced(s);
  SUB_T0();
  if constexpr (TP::REST_B > 0) {
    // (Round 1 re-used the rest's matrix factors from the smooth solve in the Newton solves.  Since the reduced problem
    // the Newton loop visits the rest only when one of its bodies is in contact — and then the factors change with the
    // contact stiffness — so every visit is a full elimination and nothing but `fact` outlives a solve.)
    if (!red) {
      if (m.rest_fast) rest_levels<TP, true, true>(s, lane, [&](const auto& nd) { rest_aba_eliminate<TP, 3>(s, nd, tau, withK, hdamp, fr, L, so, IM, m); });
      else rest_levels<TP, false, true>(s, lane, [&](const auto& nd) { rest_aba_eliminate<TP, 0>(s, nd, tau, withK, hdamp, fr, L, so, IM, m); });
      WSYNC();
    }
  }
  SUB(18);
  float IA[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float pA = 0.f;
  // ---- backward sweep along the leg.  What a hinge reads — its motion subspace, diagonal term and force, and at a body's last
  // hinge the body's inertia row — does not depend on the chain, but LDS takes a wave's operations in order and the sweep also
  // stores (the factors the contact-space solve keeps): a read issued where it is used waits for its own round trip, three
  // times per hinge.  So the reads run ONE HINGE AHEAD of the arithmetic (software pipeline, written out: the stores may alias
  // for all the compiler knows, it will not move a read across them).
  float n_sj[6], n_sown = 0.f, n_delta = 0.f, n_tau = 0.f, n_row[6];
  auto fetch_hinge = [&](auto DN) {
    constexpr int dn = decltype(DN)::value;
#pragma unroll
    for (int i = 0; i < 6; i++) n_sj[i] = Sleg[dn * SW + i];
    n_sown = Sown[dn * SW];
    n_delta = dof_delta(s, m, j0 + dn, hdamp);
    n_tau = tau[j0 + dn];
    if constexpr (TP::is_last(dn) && kHasIsym<TP>) {
#pragma unroll
      for (int c = 0; c < 6; c++) n_row[c] = s.Isym[b0 + TP::lbody(dn)][so[c]];
    }
  };
  fetch_hinge(std::integral_constant<int, TP::NDL - 1>{});
  static_for<TP::NDL>([&](auto DD) {
    constexpr int d = TP::NDL - 1 - decltype(DD)::value;
    float sj[6], row[6];
#pragma unroll
    for (int i = 0; i < 6; i++) { sj[i] = n_sj[i]; row[i] = n_row[i]; }
    const float sown = n_sown, delta = n_delta, tj = n_tau;
    if constexpr (d > 0) fetch_hinge(std::integral_constant<int, (d > 0 ? d - 1 : 0)>{});
    if constexpr (TP::is_last(d)) {          // entering a new body (going towards the root)
      const int b = b0 + TP::lbody(d);
      if constexpr (kHasIsym<TP>) {
        if constexpr (kDual<TP>) {
          if (withF) {
#pragma clang loop unroll(disable) vectorize(disable)
            for (int c = cs[TP::lbody(d)]; c < cs[TP::lbody(d) + 1]; ++c) pA -= dual_wrench(s)[c][L.rr];
          }
        }
        if (withK) for (int c = cs[TP::lbody(d)]; c < cs[TP::lbody(d) + 1]; ++c) add_contact_K_row(row, s, c, KL, fr, L.rr, walls);
        add6(IA, row);
      } else {
        add_inertia_row(IA, s, b, IM);
        if constexpr (kDual<TP>) {
          if (withF) {
#pragma clang loop unroll(disable) vectorize(disable)
            for (int c = cs[TP::lbody(d)]; c < cs[TP::lbody(d) + 1]; ++c) pA -= dual_wrench(s)[c][L.rr];
          }
        }
        if (withK) for (int c = cs[TP::lbody(d)]; c < cs[TP::lbody(d) + 1]; ++c) add_contact_K_row(IA, s, c, KL, fr, L.rr, walls);
      }
    }
    const float sr = kShadow0 ? sown : L.mask * sown;
    if constexpr (kKeepS) Sreg[d] = sown;        // shadow rows: zero (kShadow0), else row 5's (same T word, same value)
    float Uraw, invDraw;
    aba_step_scaled<kShadow0>(IA, pA, sj, sr, L.mask, delta, tj, Ureg[d], ureg[d], Uraw, invDraw);
    if constexpr (kDual<TP>) {
      if (store) {      // rows 0..5: U / sqrt D; lanes 6, 7 of the group: 1 / sqrt D
        const float rs = __builtin_sqrtf(invDraw);
        if constexpr (kDualGlob<TP>) ((__attribute__((address_space(1))) float*)s.dual_glob[0])[(L.lg * TP::NDL + d) * 8 + (L.r < 6 ? L.r : 6)] = L.r < 6 ? Uraw * rs : rs;
        else dual_leg(s)[L.lg * TP::NDL + d][L.r < 6 ? L.r : 6] = L.r < 6 ? Uraw * rs : rs;
      }
    }
  });
  // the legs' articulated inertias and bias forces meet at the root: summed over the wave's lane groups on the VALU (groups_sum;
  // the two groups that shadow the last leg contribute zero) — every group then holds the total, which is what the redundant root
  // elimination below wants.  (Until round 5 through LDS: 7 stores, then 42 reads per lane.)
  constexpr bool kLegSumValu = TP::NLEG <= 8;
  float legs_row[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, legs_pA = 0.f;
  if constexpr (kLegSumValu) {
    const float gm = L.grp < TP::NLEG ? 1.f : 0.f;
#pragma unroll
    for (int i = 0; i < 6; i++) legs_row[i] = groups_sum(gm * IA[i]);
    legs_pA = groups_sum(gm * pA);
  } else {
#pragma unroll
    for (int i = 0; i < 6; i++) H.legIA[L.lg][L.rr][i] = IA[i];
    H.legpA[L.lg][L.rr] = pA;
    WSYNC();
  }
  // ---- root: every group eliminates the six root dofs redundantly (no single-lane solve, no broadcast).
  // The free joint spans all six spatial directions, so the elimination runs in world axes (angular x, y, z about the
  // root origin, then linear x, y, z) instead of the joint's own (body-frame rotation axes): with unit axes U is a column
  // of IA, D and s.pA are single entries (one group broadcast each, and D's is one of the six U broadcasts the rank-1
  // update needs anyway) — 11 instead of 28 vector instructions per dof.  Generalized forces go in as R tau_rot, the
  // rotational accelerations come out as RT alpha.
  float Ur[6], ur[6];                   // U / D, u / D of the six root directions
  float Rm[3][3];                       // Rm[c][k] = component c of the k-th rotation axis of the free joint
  {
    float row[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if constexpr (kHasIsym<TP>) {
#pragma unroll
      for (int c = 0; c < 6; c++) row[c] = s.Isym[0][so[c]];
    } else add_inertia_row(row, s, 0, IM);
    if (withK) {
      for (int c = cs_root0; c < cs_root1; ++c) add_contact_K_row(row, s, c, KL, fr, L.rr, walls);
      // tether weld: its six rows are the components of the root twist -> a diagonal term per row
      if constexpr (WELD) static_for<6>([&](auto I) { constexpr int i = decltype(I)::value; row[i] += L.rr == i ? s.weldD[i] : 0.f; });
    }
    pA = 0.f;
    if constexpr (kDual<TP>) {
      if (withF) for (int c = cs_root0; c < cs_root1; ++c) pA -= dual_wrench(s)[c][L.rr];
    }
    if constexpr (kLegSumValu) { add6(row, legs_row); pA += legs_pA; }
    else {
#pragma unroll
      for (int k = 0; k < TP::NLEG; ++k) {
        add6(row, H.legIA[k][L.rr]);
        pA += H.legpA[k][L.rr];
      }
    }
    if constexpr (TP::REST_B > 0) {
      if (red) {
#pragma unroll
        for (int i = 0; i < 6; i++) row[i] += s.restA[so[i]];
      } else {
        // the smooth solve's factors give the reduced constraint problem its root term: the articulated inertia the rest's
        // children of the root hand over (restA), summed here while the slots are alive
        if (!withK && hdamp == 0.f && lane < 21) {
          float a = 0.f;
          for (int k = (int)s.t_cstart[0]; k < (int)s.t_cstart[0] + (int)s.t_ccount[0]; ++k) a += s.slot_at(k - 1)[lane];
          s.restA[lane] = a;
        }
        for (int k = (int)s.t_cstart[0]; k < (int)s.t_cstart[0] + (int)s.t_ccount[0]; ++k) {
          const float* sl = s.slot_at(k - 1);               // hybrid: slots in breadth-first order
          { float v[6];
#pragma unroll
            for (int i = 0; i < 6; i++) v[i] = sl[so[i]];
            add6(row, v); }
          pA += sl[21 + L.rr];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 6; i++) IA[i] = row[i];
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
      for (int c = 0; c < 3; c++) Rm[c][k] = s.S[3 + k][c];
    float tw[6];
    const float t3 = tau[3], t4 = tau[4], t5 = tau[5];
#pragma unroll
    for (int c = 0; c < 3; c++) { tw[c] = Rm[c][0] * t3 + Rm[c][1] * t4 + Rm[c][2] * t5; tw[3 + c] = tau[c]; }
    static_for<6>([&](auto DD) {
      constexpr int i = decltype(DD)::value;
      constexpr int e = i < 3 ? 2 - i : 8 - i;          // angular z, y, x, then linear z, y, x
      const float U = IA[e];
      const float b0 = grp8_bcast<0>(U), b1 = grp8_bcast<1>(U), b2 = grp8_bcast<2>(U), b3 = grp8_bcast<3>(U),
                  b4 = grp8_bcast<4>(U), b5 = grp8_bcast<5>(U);
      const float D = e == 0 ? b0 : e == 1 ? b1 : e == 2 ? b2 : e == 3 ? b3 : e == 4 ? b4 : b5;
      const float sp = grp8_bcast<e>(pA);
      const float invD = __builtin_amdgcn_rcpf(D);
      const float u = tw[e] - sp;
      const float k = U * invD;
      { const float bb[6] = {b0, b1, b2, b3, b4, b5}; fma6(IA, -k, bb); }
      pA += k * u;
      Ur[e] = kShadow0 ? k : L.mask * k; ur[e] = u * invD;
      if constexpr (kDual<TP>) {
        if (store) {
          const float rs = __builtin_sqrtf(invD);
          dual_root(s)[i][L.r < 6 ? L.r : 6] = L.r < 6 ? U * rs : rs;
        }
      }
    });
  }
  // ---- forward sweep: root (linear x, y, z, then angular x, y, z), then down the leg
  float a = 0.f;
  {
    float xw[6];
    static_for<6>([&](auto DD) {
      constexpr int i = decltype(DD)::value;
      constexpr int e = i < 3 ? 3 + i : i - 3;
      const float xe = ur[e] - grp8_sum(Ur[e] * a);
      xw[e] = xe;
      a = (kShadow0 ? L.r : L.rr) == e ? a + xe : a;
    });
#pragma unroll
    for (int k = 0; k < 3; k++) {
      x[k] = xw[3 + k];
      x[3 + k] = Rm[0][k] * xw[0] + Rm[1][k] * xw[1] + Rm[2][k] * xw[2];
    }
  }
  s.T[0][rS] = a;
  static_for<TP::NDL>([&](auto DD) {
    constexpr int d = decltype(DD)::value;
    const int j = j0 + d;
    const float xj = ureg[d] - grp8_sum(Ureg[d] * a);
    x[j] = xj;
    if constexpr (kKeepS) a += xj * Sreg[d]; else a += xj * Sown[d * SW];
    if constexpr (TP::is_last(d)) s.T[b0 + TP::lbody(d)][rS] = a;
  });
  WSYNC();
  SUB(19);
  if constexpr (TP::REST_B > 0) {
    if (!red) {
      if (m.rest_fast) rest_levels<TP, true, false>(s, lane, [&](const auto& nd) { rest_aba_expand<TP, 3, false>(s, nd, x, L); });
      else rest_levels<TP, false, false>(s, lane, [&](const auto& nd) { rest_aba_expand<TP, 0, false>(s, nd, x, L); });
    }
  }
  SUB(20);
  }
}

// ------------------------------------------------------------------ contact rows held in registers
// leg-chain kernels (star topology, no rest of the body): the passes over the dofs visit dof lane + 64 i in turn i
template <class TP> constexpr bool dual_hybrid_free() { if constexpr (TP::kStar) return TP::REST_V == 0; else return false; }
template <class TP> constexpr int spring_regs() { if constexpr (dual_hybrid_free<TP>()) return (TP::NV + kWave - 1) / kWave; else return 1; }
struct ContactRegs {
  bool on;
  V3 r;
  int body, geom, info;
  float dist, mu, D, K, B, imp, margin;
  float aref[4], jar[4], jv[4];
};

__device__ __forceinline__ float impedance(const float* si, float r) {
  float d0 = si[0], dmax = si[1], width = si[2], mid = si[3], power = si[4];
  if (d0 == dmax || width <= kMinVal) return 0.5f * (d0 + dmax);
  float x = fabsf(r) / width, y;
  if (x >= 1.f) y = 1.f;
  else if (x <= 0.f) y = 0.f;
  else if (power == 1.f) y = x;
  else if (power == 2.f) y = x <= mid ? x * x / mid : 1.f - (1.f - x) * (1.f - x) / (1.f - mid);
  else if (x <= mid) y = powf(x, power) / powf(mid, power - 1.f);
  else y = 1.f - powf(1.f - x, power) / powf(1.f - mid, power - 1.f);
  return d0 + y * (dmax - d0);
}

// Refresh the fields of the contact registers that also live in LDS.  Called right after every non-inlined
// ABA sweep so that only the row residuals (aref, jar) stay live in registers across the call.
template <class TP>
__device__ __forceinline__ void contact_reload(ContactRegs& c, const FlyLds<TP>& s, int lane) {
  if (c.on) {
    c.r = ld3(s.c_r[lane]); c.D = s.c_D[lane]; c.mu = s.c_mu[lane];
    // (the packed info word — hence the body — stays in its register across the call: the body twist the rows need next
    // is requested together with these reads instead of one LDS round trip later)
  }
}

// rows k = 0..3 :  n + mu t1, n − mu t1, n + mu t2, n − mu t2   applied to the body twist at r
__device__ __forceinline__ void rows_of_twist(const ContactRegs& c, const Frame& fr, SV t, float* out) {
  V3 vp = t.l + cross(t.a, c.r);
  float jn = dot(fr.n, vp), j1 = c.mu * dot(fr.t1, vp), j2 = c.mu * dot(fr.t2, vp);
  out[0] = jn + j1; out[1] = jn - j1; out[2] = jn + j2; out[3] = jn - j2;
}

// One row of the tether weld (TetheredWorld): lanes 48..53 own the six bilateral rows, which are the components
// (w; v) of the root twist, so J x is a component of T[0] and JT f a component of the root wrench.
struct WeldRow { bool on; int comp; float D, aref, jar, jv; };

// this lane's share of the constraint cost (callers that have other wave sums to take put them in one reduction round)
__device__ __forceinline__ float constraint_cost_lane(const ContactRegs& c, const WeldRow& wr) {
  float v = wr.on ? 0.5f * wr.D * wr.jar * wr.jar : 0.f;
  if (c.on) {
#pragma unroll
    for (int k = 0; k < 4; k++) if (c.jar[k] < 0.f) v += 0.5f * c.D * c.jar[k] * c.jar[k];
  }
  return v;
}
template <class TP>
__device__ float constraint_cost(const ContactRegs& c, const WeldRow& wr) {
  float v = wr.on ? 0.5f * wr.D * wr.jar * wr.jar : 0.f;
  if (c.on) {
#pragma unroll
    for (int k = 0; k < 4; k++) if (c.jar[k] < 0.f) v += 0.5f * c.D * c.jar[k] * c.jar[k];
  }
  return wave_sum(v);
}

// emit(j, (JT rows)_j [+ seed_scale * (subtree sum of W)_j])  for per-contact row forces `rows` (pyramid rows of the
// lane's contact) and the tether row force `weld_row`: every contact lane publishes its world wrench (about the
// root origin) in c_w, then the leg groups suffix-sum the wrenches of their bodies' contacts (contacts are sorted by
// body) and the dofs project.  SEEDED: W already holds per-body wrenches (I_b T_b of the search direction) that ride
// the same sweep, so  alpha M search − JT df  costs one pass.  The active-row mask of c.jar goes to c_info for the ABA.
template <class TP, bool SEEDED, class Emit>
__device__ __forceinline__ void contact_sweep(FlyLds<TP>& s, float seed_scale, const GModel& m, int lane, Emit&& emit);
template <class TP, bool SEEDED, class Emit>
__device__ __forceinline__ void contact_project(FlyLds<TP>& s, const ContactRegs& c, const WeldRow& wr, const Frame& fr,
                                                const float* rows, float weld_row, float seed_scale,
                                                const GModel& m, int lane, bool walls, Emit&& emit) {
  if (wr.on) s.weld_w[wr.comp] = weld_row;
  if (c.on) {
    int act = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) act |= (c.jar[k] < 0.f ? 1 : 0) << k;
    float fn = rows[0] + rows[1] + rows[2] + rows[3], f1 = c.mu * (rows[0] - rows[1]), f2 = c.mu * (rows[2] - rows[3]);
    V3 F;
    if (walls) { const Frame cf = contact_frame(info_fid(c.info), fr); F = fn * cf.n + f1 * cf.t1 + f2 * cf.t2; }
    else F = fn * fr.n + f1 * fr.t1 + f2 * fr.t2;
    stsv(s.c_w[lane], SV{cross(c.r, F), F});
    s.c_info[lane] = c.info | (act << 20);
    if constexpr (kHasCm3<TP>) {
      const float a0 = (act & 1) ? 1.f : 0.f, a1 = (act & 2) ? 1.f : 0.f, a2 = (act & 4) ? 1.f : 0.f, a3 = (act & 8) ? 1.f : 0.f;
      const float Dm = c.D * c.mu, Dmm = Dm * c.mu;
      float* q = s.c_m3[lane];
      q[0] = c.D * (a0 + a1 + a2 + a3); q[1] = Dm * (a0 - a1); q[2] = Dm * (a2 - a3); q[3] = Dmm * (a0 + a1); q[4] = Dmm * (a2 + a3);
    }
  }
  WSYNC();
  contact_sweep<TP, SEEDED>(s, seed_scale, m, lane, emit);
}
// the second half of contact_project: the contact wrenches are in c_w (and the tether's in weld_w)
template <class TP, bool SEEDED, class Emit>
__device__ __forceinline__ void contact_sweep(FlyLds<TP>& s, float seed_scale, const GModel& m, int lane, Emit&& emit) {
  if constexpr (!TP::kStar) {
    tree_sweep_project(s, s.W, m, lane, [&](int b, SV w) {
      SV own = SEEDED ? seed_scale * w : SV{v3(0.f, 0.f, 0.f), v3(0.f, 0.f, 0.f)};
      if (b == 0) own = own + ldsv(s.weld_w);
      for (int cc = s.body_cstart[b]; cc < s.body_cstart[b + 1]; ++cc) own = own + ldsv(s.c_w[cc]);
      return own;
    }, emit);
    return;
  } else {
  const bool red = rest_reduced(s);
  if constexpr (TP::REST_B > 0) {    // head / abdomen / wing contacts: tree levels of the rest of the body
    if (!red) tree_gather_levels(s, s.W, m, lane, [&](int b, SV w) {
      SV own = SEEDED ? seed_scale * w : SV{v3(0.f, 0.f, 0.f), v3(0.f, 0.f, 0.f)};
      for (int cc = s.body_cstart[b]; cc < s.body_cstart[b + 1]; ++cc) own = own + ldsv(s.c_w[cc]);
      return own;
    });
  }
  const LaneRole L = lane_role<TP>(lane);
  const int b0 = TP::LB0 + L.lg * TP::NBL;
  float acc = 0.f;
  int cs[TP::NBL + 1];                       // contact ranges of the leg's bodies, fetched in one batch
  static_for<TP::NBL + 1>([&](auto I) { constexpr int l = decltype(I)::value; cs[l] = s.body_cstart[b0 + l]; });
  static_for<TP::NBL>([&](auto I) {
    constexpr int l = TP::NBL - 1 - decltype(I)::value;
    if (SEEDED) acc += seed_scale * s.W[b0 + l][L.rr];
    for (int cc = cs[l]; cc < cs[l + 1]; ++cc) acc += s.c_w[cc][L.rr];
    s.W[b0 + l][L.rr] = acc;
  });
  WSYNC();
  if (lane < 6) {
    float a0 = s.weld_w[lane];
    if (SEEDED) a0 += seed_scale * s.W[0][lane];
    for (int cc = s.body_cstart[0]; cc < s.body_cstart[1]; ++cc) a0 += s.c_w[cc][lane];
#pragma unroll
    for (int k = 0; k < TP::NLEG; ++k) a0 += s.W[TP::LB0 + k * TP::NBL][lane];
    if constexpr (TP::REST_B > 0) {
      if (!red) for (int k = (int)s.t_cstart[0]; k < (int)s.t_cstart[0] + (int)s.t_ccount[0]; ++k) a0 += s.W[(int)s.t_body[k]][lane];
    }
    s.W[0][lane] = a0;
  }
  WSYNC();
  for_dofs(s, red, lane, [&](int j) {
    emit(j, dot(ldsv(s.S[j]), ldsv(s.W[j >= TP::LD0 || j < 6 ? dof_body_of<TP>(j) : tbl_dofbody(s, j)])));
  });
  WSYNC();
  }
}

// row forces f_k = −D jar_k on the active (jar < 0) pyramid rows, times `sign`
__device__ __forceinline__ void contact_row_forces(const ContactRegs& c, float sign, float* f) {
#pragma unroll
  for (int k = 0; k < 4; k++) f[k] = c.jar[k] < 0.f ? -sign * c.D * c.jar[k] : 0.f;
}

}  // namespace nmf
#include "nmf_dual.h"
namespace nmf {

// ------------------------------------------------------------------ noslip post-pass on the primal path
// option/noslip_iterations of the CPU flavour (reference mujoco_globals.yaml:15 under mujoco.mj_step, src/flygym/simulation.py:74-76;
// restated from MuJoCo's documentation in oracle/nmf_oracle.c::noslip) for every step the contact-space solve — where the pass
// is a few wave sums over G — does not take: the full-body and general-tree skeletons, tethered worlds, steps with more than
// sixteen contacts.  One world, so cost is no object: A = J M^-1 J^T is built column by column with one articulated-body solve
// per constraint row (a unit force on the row, pushed to the dofs, solved, read back through every row) into the world's
// scratch in HBM (DevState::noslip_buf: [198][198] columns by fixed row ids — contact c row k = 4 c + k, tether row i = 192 + i —
// then the rows' reference accelerations, stored when they were computed, then this function's result); then the same pair
// Gauss-Seidel as the oracle's — (f0, f1) = (mid + y, mid - y), y in [-mid, mid] minimises 1/2 f^T A f + f^T b, an update that
// raises the cost is undone, up to noslip_iter sweeps — lane = contact, its four forces in registers.  The caller turns the
// forces into J^T f and qacc.  Its own function: nothing of it may sit in the stepping kernels' registers.
constexpr int kNoslipRows = 4 * kMaxCon + 6;
constexpr int kNoslipFloats = kNoslipRows * (kNoslipRows + 2);
template <class TP, bool WELD>
__device__ __noinline__ void noslip_primal(FlyLds<TP>& s, const GModel& m, int lane, float* __restrict__ buf, int ncon, bool walls,
                                           bool con, int cinfo, float q0, float q1, float q2, float q3, float wforce, float wD) {
  constexpr int NR = kNoslipRows;
  const Frame fr = make_frame(v3(m.plane[0], m.plane[1], m.plane[2]));
  ContactRegs c{};
  c.on = con; c.info = cinfo; c.body = info_body(cinfo); c.geom = info_geom(cinfo);
  contact_reload(c, s, lane);
  WeldRow wr{};
  wr.comp = lane - 48;
  wr.on = WELD && wr.comp >= 0 && wr.comp < 6;
  auto rows = [&](SV t, float* out) {
    if (walls) rows_of_twist(c, contact_frame(info_fid(c.info), fr), t, out); else rows_of_twist(c, fr, t, out);
  };
  float f[4] = {q0, q1, q2, q3};
  // b = J qacc_smooth - aref
  sweep_twists(s, s.qacc_smooth, s.T, m, lane);
  float b[4] = {0.f, 0.f, 0.f, 0.f};
  if (c.on) {
    rows(ldsv(s.T[c.body]), b);
#pragma unroll
    for (int k = 0; k < 4; ++k) b[k] -= buf[NR * NR + 4 * lane + k];
  }
  WSYNC();
  const int nrow_c = 4 * ncon;
  for (int i = 0; i < nrow_c + (WELD ? 6 : 0); ++i) {
    const bool isw = i >= nrow_c;
    const int ci = i >> 2, ki = i & 3, wc = i - nrow_c;
    float e[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) e[k] = (!isw && lane == ci && k == ki) ? 1.f : 0.f;
    const float ew = isw && wr.comp == wc ? 1.f : 0.f;
    contact_project<TP, false>(s, c, wr, fr, e, ew, 0.f, m, lane, walls, [&](int j, float v) { s.vA[j] = v; });
    aba_solve<TP, WELD>(s, V_A, V_B, false, 0.f, m, lane);       // T = twists(M^-1 J_i^T)
    contact_reload(c, s, lane);
    const int col = isw ? 4 * kMaxCon + wc : i;
    if (c.on) {
      float a[4];
      rows(ldsv(s.T[c.body]), a);
#pragma unroll
      for (int k = 0; k < 4; ++k) buf[col * NR + 4 * lane + k] = a[k];
    }
    if (wr.on) buf[col * NR + 4 * kMaxCon + wr.comp] = s.T[0][wr.comp];
    WSYNC();
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");      // the columns are read across lanes through memory
  const float scale = 1.0f / (m.meaninertia * (float)s.nv());
  for (int sweep = 0; sweep < m.noslip_iter; ++sweep) {
    float improvement = 0.f;
    if (sweep == 0) {      // the regulariser's share of the cost drops out
      float v = 0.f;
      if (c.on) { const float rD = 1.0f / c.D; v = 0.5f * rD * (f[0] * f[0] + f[1] * f[1] + f[2] * f[2] + f[3] * f[3]); }
      if (wr.on && wD > 0.f) v += 0.5f * wforce * wforce / wD;
      improvement = wave_sum(v);
    }
    for (int c2 = 0; c2 < ncon; ++c2) {
      for (int pp = 0; pp < 2; ++pp) {
        const int r0 = 4 * c2 + 2 * pp, r1 = r0 + 1;
        float p0 = 0.f, p1 = 0.f;
        if (c.on) {
#pragma unroll
          for (int k = 0; k < 4; ++k) { p0 = fmaf(buf[r0 * NR + 4 * lane + k], f[k], p0); p1 = fmaf(buf[r1 * NR + 4 * lane + k], f[k], p1); }
        }
        if (wr.on) { p0 = fmaf(buf[r0 * NR + 4 * kMaxCon + wr.comp], wforce, p0); p1 = fmaf(buf[r1 * NR + 4 * kMaxCon + wr.comp], wforce, p1); }
        const float res0 = wave_sum(p0) + readlane_f(pp == 0 ? b[0] : b[2], c2), res1 = wave_sum(p1) + readlane_f(pp == 0 ? b[1] : b[3], c2);
        const float a00 = buf[r0 * NR + r0], a01 = buf[r0 * NR + r1], a11 = buf[r1 * NR + r1];
        const float old0 = readlane_f(pp == 0 ? f[0] : f[2], c2), old1 = readlane_f(pp == 0 ? f[1] : f[3], c2);
        const float bc0 = res0 - a00 * old0 - a01 * old1, bc1 = res1 - a01 * old0 - a11 * old1;
        const float mid = 0.5f * (old0 + old1);
        const float K1 = a00 + a11 - 2.f * a01, K0 = mid * (a00 - a11) + bc0 - bc1;
        float n0 = mid, n1 = mid;
        if (!(K1 < kMinVal)) { const float y = fminf(fmaxf(-K0 / K1, -mid), mid); n0 = mid + y; n1 = mid - y; }
        const float d0 = n0 - old0, d1 = n1 - old1;
        float change = 0.5f * (d0 * (a00 * d0 + a01 * d1) + d1 * (a01 * d0 + a11 * d1)) + d0 * res0 + d1 * res1;
        if (change > 1e-10f) { n0 = old0; n1 = old1; change = 0.f; }
        if (lane == c2) { if (pp == 0) { f[0] = n0; f[1] = n1; } else { f[2] = n0; f[3] = n1; } }
        improvement -= change;
      }
    }
    if (scale * improvement < 1e-6f) break;          // noslip_tolerance (MuJoCo's default)
  }
  if (c.on) {
#pragma unroll
    for (int k = 0; k < 4; ++k) buf[NR * NR + NR + 4 * lane + k] = f[k];
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
}

// The control-table row of the NEXT step, requested from inside the current one.  Every non-inlined stage function begins
// with `s_waitcnt vmcnt(0)` (the calling convention: a callee cannot know what is in flight), so a load issued right before
// a call — round 2 requested the row at the top of the step, just ahead of the kinematics call — is waited for at once, HBM
// latency and all, every step.  physics_forward issues it right after the collision stage returns: ~8 k cycles of inlined
// work (contact parameters, velocities, bias forces, actuation) follow before the next call.
struct CtrlPrefetch {
  const float* next_row;    // table row of the next step (nullptr: none)
  bool mine;                // this lane carries a column
  float value;              // the lane's entry of that row, once loaded
};

// ------------------------------------------------------------------ the step
// ------------------------------------------------------------------ general actuators (cold: models that have them)
// MuJoCo's general actuator for the reference's ActuatorType members beyond the stateless affine ones — intvelocity, damper,
// cylinder, muscle (reference compose/fly.py:65-77, 301-369 forwards the MJCF shortcut; oracle: nmf_oracle.c general_actuator,
// same formulas) — and for the second and later actuators of a dof that several drive.  The affine pass of physics_forward sees
// these as motors of gain 0; this pass, one lane per actuator, computes force = gain(length, velocity) * input + bias(length,
// velocity), input = the control or — stateful types — the activation at the START of the step (mj_fwdActuation, option actearly
// off), clamps it, adds gear * force to the dof's direct force (an LDS atomic: dofs may be shared) and writes the NEXT activation
// (mj_advance: act + h act_dot, filterexact's closed form, clamped to actrange) to the world's slot in HBM — nothing else in the step
// reads it.  Off the hot path: a wave-uniform branch on m.act_general skips it for every model of BASELINE.json.
constexpr int kActGen = 32;       // floats per actuator in DevModel::act_general (flygym_amd/compiler/model.py::_general_row)
__device__ __forceinline__ float muscle_peak(const float* prm, float acc0) { return prm[2] < 0.f ? prm[3] / fmaxf(kMinVal, acc0) : prm[2]; }
__device__ __forceinline__ float muscle_len(float len, float lr0, float lr1, const float* prm, float& L0) {
  L0 = (lr1 - lr0) / fmaxf(kMinVal, prm[1] - prm[0]);
  return prm[0] + (len - lr0) / fmaxf(kMinVal, L0);
}
template <class TP>
__device__ __noinline__ void actuation_general(FlyLds<TP>& s, const GModel& m, int lane, float* __restrict__ act_w, float* __restrict__ force_out,
                                               float* __restrict__ rec_out, int rec_n) {
  typedef __attribute__((address_space(3))) float* lds_fptr;
  const float h = m.timestep;
  for (int u = lane; u < m.nu; u += kWave) {
    const NMF_G float* g = m.act_general + (size_t)u * kActGen;
    const int flags = (int)g[0];
    if (!(flags & 1)) continue;
    float prm[26];
#pragma unroll
    for (int i = 0; i < 26; ++i) prm[i] = g[6 + i];          // dynprm 0..2 | gainprm 3..11 | biasprm 12..20 | actrange 21, 22 | lengthrange 23, 24 | acc0 25
    const int dyn = (int)g[1], gt = (int)g[2], bt = (int)g[3];
    const float gear = g[5];
    float ctrl = s.ctrl[u];
    if (m.act_limited[2 * u + 1]) ctrl = fminf(fmaxf(ctrl, m.act_ctrlrange[2 * u]), m.act_ctrlrange[2 * u + 1]);
    const int j = flags >> 8;        // (the uploaded act_trn points these actuators at dof 0: see nmf_batch_create)
    const float len = gear * s.qpos[j + 1], vel = gear * s.qvel[j];
    const float act = dyn ? act_w[u] : 0.f;
    if (dyn) {
      float act_dot;
      if (dyn == 1) act_dot = ctrl;
      else if (dyn == 4) {
        const float cc = fminf(fmaxf(ctrl, 0.f), 1.f), ac = fminf(fmaxf(act, 0.f), 1.f);
        const float ta = prm[0] * (0.5f + 1.5f * ac), td = prm[1] / (0.5f + 1.5f * ac), dc = cc - act;
        float tau;
        if (prm[2] < kMinVal) tau = dc > 0.f ? ta : td;
        else {
          const float x = dc / prm[2] + 0.5f;
          const float sg = x <= 0.f ? 0.f : (x >= 1.f ? 1.f : x * x * x * (3.f * x * (2.f * x - 5.f) + 10.f));
          tau = td + (ta - td) * sg;
        }
        act_dot = dc / fmaxf(kMinVal, tau);
      } else act_dot = (ctrl - act) / fmaxf(kMinVal, prm[0]);
      float nx;
      if (dyn == 3) { const float tau = fmaxf(kMinVal, prm[0]); nx = act + act_dot * tau * (1.f - expf(-h / tau)); }
      else nx = act + act_dot * h;
      if (g[4] != 0.f) nx = fminf(fmaxf(nx, prm[21]), prm[22]);
      act_w[u] = nx;
    }
    const float input = dyn ? act : ctrl;
    const float* gp = prm + 3;
    const float* bp = prm + 12;
    float gain, f;
    if (gt == 2) {
      float L0;
      const float L = muscle_len(len, prm[23], prm[24], gp, L0);
      const float V = vel / fmaxf(kMinVal, L0 * gp[6]);
      const float lmin = gp[4], lmax = gp[5], fvmax = gp[8];
      const float a = 0.5f * (lmin + 1.f), b = 0.5f * (1.f + lmax);
      float FL = 0.f, FV, x;
      if (L >= lmin && L <= a) { x = (L - lmin) / fmaxf(kMinVal, a - lmin); FL = 0.5f * x * x; }
      else if (L > a && L <= 1.f) { x = (1.f - L) / fmaxf(kMinVal, 1.f - a); FL = 1.f - 0.5f * x * x; }
      else if (L > 1.f && L <= b) { x = (L - 1.f) / fmaxf(kMinVal, b - 1.f); FL = 1.f - 0.5f * x * x; }
      else if (L > b && L <= lmax) { x = (lmax - L) / fmaxf(kMinVal, lmax - b); FL = 0.5f * x * x; }
      const float y = fvmax - 1.f;
      if (V <= -1.f) FV = 0.f;
      else if (V <= 0.f) FV = (V + 1.f) * (V + 1.f);
      else if (V <= y) FV = fvmax - (y - V) * (y - V) / fmaxf(kMinVal, y);
      else FV = fvmax;
      gain = -muscle_peak(gp, prm[25]) * FL * FV;
    } else gain = gt == 1 ? gp[0] + gp[1] * len + gp[2] * vel : gp[0];
    f = gain * input;
    if (bt == 1) f += bp[0] + bp[1] * len + bp[2] * vel;
    else if (bt == 2) {
      float L0;
      const float L = muscle_len(len, prm[23], prm[24], bp, L0);
      const float lmax = bp[5], fpmax = bp[7], b = 0.5f * (1.f + lmax);
      float FP = 0.f;
      if (L > 1.f && L <= b) { const float x = (L - 1.f) / fmaxf(kMinVal, b - 1.f); FP = fpmax * 0.5f * x * x; }
      else if (L > b) { const float x = (L - b) / fmaxf(kMinVal, b - 1.f); FP = fpmax * (0.5f + x); }
      f -= muscle_peak(bp, prm[25]) * FP;
    }
    if (flags & 2) f = fminf(fmaxf(f, m.act_forcerange[2 * u]), m.act_forcerange[2 * u + 1]);
    (void)__hip_atomic_fetch_add((lds_fptr)(void*)&s.vA[j], gear * f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (force_out) force_out[u] = f;
    if (rec_out && u < rec_n) rec_out[u] = f;
  }
  WSYNC();
}

template <class TP, bool WELD>
__device__ bool physics_forward(FlyLds<TP>& s, const GModel& m, int lane, const DevState& st, int w, bool last, float* rec, CtrlPrefetch& pf STAGE_ARG) {
  // hybrid kernels: per-lane addresses are rebuilt every step instead of living across the item loop — hoisted, they left
  // the 132-dof kernel 19 spilled registers and a dozen scratch reloads per step (the 72-dof kernels have the registers to
  // keep them: recomputing costs those 2 %)
  // (the leg-chain terrain kernels likewise: their per-contact frames take the registers the flat kernels keep the addresses in)
  if constexpr (TP::kStar) { if constexpr (TP::REST_B > 0 || TP::kTerrain) lane = opaque(lane); }
  const Frame fr = make_frame(v3(m.plane[0], m.plane[1], m.plane[2]));
  if constexpr (TP::kStar) { if constexpr (TP::REST_B > 0) { if (lane == 0) s.reduced = 0; } }
  stage_kinematics(s, m, lane);
  STAGE(1);
  stage_inertia(s, m, lane);
  STAGE(2);
  stage_collision<TP, TP::kTerrain>(s, m, lane);
  if (pf.next_row && pf.mine) pf.value = G(pf.next_row)[lane];      // consumed at the top of the next step
  if (last) write_poses(s, m, st, w, lane);       // the body poses die here (their LDS is the solver's from now on)
  STAGE(3);
  const int ncon = s.ncon;
  // terrain side faces in contact this step: those contacts carry their own frames (wave-uniform; flat worlds: never)
  const bool walls = TP::kTerrain && __builtin_amdgcn_readfirstlane(s.nwall) != 0;

  // ---- contact parameters (lane c owns contact c)
  ContactRegs c;
  auto rows = [&](SV t, float* out) {       // the four pyramid rows of this lane's contact applied to a body twist
    if (walls) rows_of_twist(c, contact_frame(info_fid(c.info), fr), t, out); else rows_of_twist(c, fr, t, out);
  };
  c.on = lane < ncon;
  // the contact's pair parameters come from the model (L2): loaded here, turned into the row constants behind the first velocity
  // pass (leg-chain kernels), which needs none of them
  float cp_solref[2] = {0.f, 0.f}, cp_solimp[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, cp_tran = 0.f;
  int cp_info0 = 0;
  if (c.on) {
    cp_info0 = s.c_info[lane];
    c.r = ld3(s.c_r[lane]); c.body = info_body(cp_info0); c.geom = info_geom(cp_info0); c.dist = s.c_D[lane];
    const int g = c.geom;
    c.info = info_pack(g, m.geom_sensor[g], c.body, 0) | (cp_info0 & (7 << 24));      // the contact's frame id stays with it
    c.mu = m.pair_friction[5 * g];
    c.margin = m.pair_margin[g];
    cp_solref[0] = m.pair_solref[2 * g]; cp_solref[1] = m.pair_solref[2 * g + 1];
#pragma unroll
    for (int i = 0; i < 5; ++i) cp_solimp[i] = m.pair_solimp[5 * g + i];
    cp_tran = m.geom_invweight0[g];
  }
  auto contact_constants = [&]() {
    if (!c.on) return;
    const float* solref = cp_solref;
    const float* solimp = cp_solimp;
    float r = c.dist - c.margin;
    c.imp = impedance(solimp, r);
    float tran = cp_tran;
    float diagA = tran + c.mu * c.mu * tran;
    float Rn = fmaxf((1.f - c.imp) * diagA / c.imp, kMinVal);
    float Rpy = fmaxf(m.sem_pyramid_plain ? Rn : 2.f * c.mu * c.mu * Rn, kMinVal);
    c.D = 1.0f / Rpy;
    float tc = solref[0], dr = solref[1];
    if (tc > 0.f) {
      tc = fmaxf(tc, 2.f * m.timestep);
      float dmax = solimp[1];
      c.K = 1.0f / (dmax * dmax * tc * tc * dr * dr);
      c.B = 2.0f / (dmax * tc);
    } else { c.K = -tc / (solimp[1] * solimp[1]); c.B = -dr / solimp[1]; }
    s.c_D[lane] = c.D; s.c_mu[lane] = c.mu; s.c_info[lane] = c.info;
  };

  // ---- tether weld rows (lanes 48..53); without a tether their stiffness and wrench are zero
  WeldRow wr;
  wr.comp = lane - 48;
  wr.on = WELD && wr.comp >= 0 && wr.comp < 6;
  wr.D = 0.f; wr.aref = 0.f; wr.jar = 0.f; wr.jv = 0.f;
  float weld_res = 0.f, weld_KI = 0.f, weld_B = 0.f;
  if (wr.comp >= 0 && wr.comp < 6) {
    if (wr.on) {
      const Q4 qe = qmul(qnorm(ldq(&s.qpos[3])), Q4{m.weld_quat[0], -m.weld_quat[1], -m.weld_quat[2], -m.weld_quat[3]});
      const float sg = qe.w < 0.f ? -2.f : 2.f;
      const float res6[6] = {sg * qe.x, sg * qe.y, sg * qe.z, s.qpos[0] - m.weld_pos[0], s.qpos[1] - m.weld_pos[1], s.qpos[2] - m.weld_pos[2]};
#pragma unroll
      for (int i = 0; i < 6; i++) weld_res = wr.comp == i ? res6[i] : weld_res;
      const float imp = impedance(m.weld_solimp, weld_res);
      const float dA = m.weld_invweight[wr.comp < 3 ? 1 : 0];
      wr.D = 1.0f / fmaxf((1.f - imp) * dA / imp, kMinVal);
      float tc = m.weld_solref[0], dr = m.weld_solref[1], K;
      const float dmax = m.weld_solimp[1];
      if (tc > 0.f) { tc = fmaxf(tc, 2.f * m.timestep); K = 1.0f / (dmax * dmax * tc * tc * dr * dr); weld_B = 2.0f / (dmax * tc); }
      else { K = -tc / (dmax * dmax); weld_B = -dr / dmax; }
      weld_KI = K * imp;
    }
    s.weldD[wr.comp] = wr.D;
    s.weld_w[wr.comp] = 0.f;
  }
  STAGE(4);
  // ---- launch constants the actuation and passive-force passes need (the lane's actuator, its dofs' springs): loaded here, a
  // stage ahead of their use — the round trip to L2 runs behind the velocity passes instead of in front of the actuation
  struct ActModel { int lim_f, lim_c, type, trn; float gain, b0, b1, c0, c1, f0, f1; };
  auto load_act = [&](int u) {
    ActModel a;
    a.lim_f = m.act_limited[2 * u]; a.lim_c = m.act_limited[2 * u + 1]; a.type = m.act_type[u]; a.trn = m.act_trn[u];
    a.gain = m.act_gain[u]; a.b0 = m.act_bias[2 * u]; a.b1 = m.act_bias[2 * u + 1];
    a.c0 = m.act_ctrlrange[2 * u]; a.c1 = m.act_ctrlrange[2 * u + 1]; a.f0 = m.act_forcerange[2 * u]; a.f1 = m.act_forcerange[2 * u + 1];
    return a;
  };
  ActModel act0{};
  if (lane < m.nu) act0 = load_act(lane);
  constexpr bool kSpringPre = dual_hybrid_free<TP>();              // leg-chain kernels (the hybrids' passes over the dofs are compacted: not lane + 64 i)
  constexpr int kSpringN = spring_regs<TP>();
  float spring_k[kSpringN], spring_ref[kSpringN];
  if constexpr (kSpringPre) {
#pragma unroll
    for (int i = 0; i < kSpringN; ++i) {
      const int j = lane + kWave * i;
      spring_k[i] = j < TP::NV ? m.dof_stiffness[j] : 0.f; spring_ref[i] = j < TP::NV ? m.dof_springref[j] : 0.f;
    }
  }
  // ---- velocities and bias accelerations: three passes over the chains
  // (CPU flavour: the rows' reference accelerations also go to the world's noslip scratch — noslip_primal reads them back)
  float* const nsbuf = m.noslip_iter > 0 && st.noslip_buf ? st.noslip_buf + (size_t)w * kNoslipFloats : nullptr;
  auto stash_aref = [&]() {
    if (!nsbuf) return;
    if (c.on) {
#pragma unroll
      for (int k = 0; k < 4; k++) nsbuf[kNoslipRows * kNoslipRows + 4 * opaque(lane) + k] = c.aref[k];
    }
  };
  if constexpr (!TP::kStar) {
    contact_constants();
    tree_velocity_bias(s, m, lane);
    if (c.on) {
      float velrow[4];
      rows(ldsv(s.W[c.body]), velrow);
      const float rr0 = c.dist - c.margin;
#pragma unroll
      for (int k = 0; k < 4; k++) c.aref[k] = -c.B * velrow[k] - c.K * c.imp * rr0;
    }
    stash_aref();
    if (wr.on) wr.aref = -weld_B * s.W[0][wr.comp] - weld_KI * weld_res;
  } else {
    // hybrid: root + the rest of the body by tree levels first (the chain passes below redo the root identically)
    if constexpr (TP::REST_B > 0) tree_velocity_bias(s, m, lane);
    const LaneRole L = lane_role<TP>(lane);
    const int j0 = TP::LD0 + L.lg * TP::NDL, b0 = TP::LB0 + L.lg * TP::NBL;
    float(*vb)[6] = reinterpret_cast<float(*)[6]>(&s.qacc_smooth[0]);   // NV x 6 floats: qacc_smooth .. vD
    // pass 1: component-wise prefix of velocities
    float vt = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) vt += s.qvel[j] * s.S[j][L.rr];
    float v = vt;
#pragma unroll
    for (int j = 3; j < 6; ++j) { if (lane < 6) vb[j][lane] = vt; v += s.qvel[j] * s.S[j][L.rr]; }
    if (lane < 6) s.W[0][lane] = v;
    {
      // (the chain's inputs first: LDS takes a wave's operations in order, so a read issued behind the chain's stores waits
      // for its own round trip at every hinge)
      float pq[TP::NDL];
#pragma unroll
      for (int d = 0; d < TP::NDL; ++d) pq[d] = s.qvel[j0 + d] * s.S[j0 + d][L.rr];
      static_for<TP::NDL>([&](auto D) {
        constexpr int d = decltype(D)::value;
        vb[j0 + d][L.rr] = v;
        v += pq[d];
        if constexpr (TP::is_last(d)) s.W[b0 + TP::lbody(d)][L.rr] = v;
      });
    }
    WSYNC();
    contact_constants();
    // reference acceleration of the contact rows needs the body velocities (still in W here)
    if (c.on) {
      float velrow[4];
      rows(ldsv(s.W[c.body]), velrow);
      const float rr0 = c.dist - c.margin;
#pragma unroll
      for (int k = 0; k < 4; k++) c.aref[k] = -c.B * velrow[k] - c.K * c.imp * rr0;
    }
    stash_aref();
    if (wr.on) wr.aref = -weld_B * s.W[0][wr.comp] - weld_KI * weld_res;
    // pass 2: per dof, Sdot_j qd_j = (v_before x S_j) qd_j
    if constexpr (dual_hybrid_free<TP>() && TP::NV - 3 > kWave && TP::NV - 3 <= 2 * kWave) {
      // (leg-chain kernels: 69 dofs are two turns of the wave, the second for five lanes — both turns' reads are issued before
      // the first turn's stores, which the second's reads may alias for all the compiler knows)
      const int ja = 3 + lane, jb = 3 + lane + kWave;
      const bool two = jb < TP::NV;
      const SV ra = s.qvel[ja] * cross_motion(ldsv(vb[ja]), ldsv(s.S[ja]));
      SV rb = ra;
      if (two) rb = s.qvel[jb] * cross_motion(ldsv(vb[jb]), ldsv(s.S[jb]));
      stsv(vb[ja], ra);
      if (two) stsv(vb[jb], rb);
    } else {
      for (int j = 3 + lane; j < s.nv(); j += kWave)
        if (TP::REST_V == 0 || j < 6 || j >= TP::LD0) stsv(vb[j], s.qvel[j] * cross_motion(ldsv(vb[j]), ldsv(s.S[j])));
    }
    WSYNC();
    // pass 3: component-wise prefix of bias accelerations (root parent acceleration = -gravity)
    float a = L.rr >= 3 ? -m.gravity[L.rr - 3] : 0.f;
#pragma unroll
    for (int j = 3; j < 6; ++j) a += vb[j][L.rr];
    if (lane < 6) s.T[0][lane] = a;
    {
      float pv[TP::NDL];
#pragma unroll
      for (int d = 0; d < TP::NDL; ++d) pv[d] = vb[j0 + d][L.rr];
      static_for<TP::NDL>([&](auto D) {
        constexpr int d = decltype(D)::value;
        a += pv[d];
        if constexpr (TP::is_last(d)) s.T[b0 + TP::lbody(d)][L.rr] = a;
      });
    }
  }
  WSYNC();
  for (int b = lane; b < s.nb(); b += kWave) {
    SV v = ldsv(s.W[b]);
    SV f = inert_mul(s.Ib[b], ldsv(s.T[b])) + cross_force(v, inert_mul(s.Ib[b], v));
    stsv(s.W[b], -1.0f * f);
  }
  for (int j = lane; j < s.nv(); j += kWave) s.vA[j] = 0.f;  // direct actuator forces
  WSYNC();
  STAGE(5);
  // ---- actuation
  for (int u = lane; u < m.nu; u += kWave) {
    const ActModel am = u < kWave ? act0 : load_act(u);
    float ctrl = s.ctrl[u];
    if (am.lim_c) ctrl = fminf(fmaxf(ctrl, am.c0), am.c1);
    float f;
    if (am.type == ACT_ADHESION) {
      f = am.gain * ctrl;
      // pulls through the contacts of the adhesion segment's own geom (the MJCF body the actuator names, reference
      // fly.py:434-439); sem_adhesion_fused: through every contact of the dynamic body the segment was merged into
      const int body = am.trn, ag = m.sem_adhesion_fused ? -2 : m.act_geom[u];
      const int c0 = s.body_cstart[body], c1 = s.body_cstart[body + 1];
      int cnt = 0;
      for (int cc = c0; cc < c1; ++cc) cnt += (ag == -2 || info_geom(s.c_info[cc]) == ag) ? 1 : 0;
      if (cnt > 0) {
        float k = -f / (float)cnt;
        SV acc = ldsv(s.W[body]);
        for (int cc = c0; cc < c1; ++cc) {
          if (ag != -2 && info_geom(s.c_info[cc]) != ag) continue;
          V3 r = ld3(s.c_r[cc]);
          const V3 nn = walls ? contact_frame(info_fid(s.c_info[cc]), fr).n : fr.n;      // along the contact's own normal
          acc = acc + k * SV{cross(r, nn), nn};
        }
        stsv(s.W[body], acc);
      }
    } else {
      int j = am.trn;
      f = am.gain * ctrl + am.b0 * s.qpos[j + 1] + am.b1 * s.qvel[j];
      if (am.lim_f) f = fminf(fmaxf(f, am.f0), am.f1);
      s.vA[j] += f;
    }
    if (last) st.actuator_force[(size_t)w * m.nu + opaque(u)] = f;     // pure output: only the launch's last step stores it
    if (rec && u < st.ring_nact) rec[2 * st.ring_nj + opaque(u)] = f;  // ... and the steps an observation ring records
  }
  WSYNC();
  if (m.act_general)      // wave-uniform: models with intvelocity / damper / cylinder / muscle actuators, or dofs that several actuators drive
    actuation_general(s, m, lane, st.act + (size_t)w * m.nu, last ? st.actuator_force + (size_t)w * m.nu : nullptr,
                      rec ? rec + 2 * st.ring_nj : nullptr, st.ring_nact);
  sweep_project(s, s.W, m, lane, [&](int j, float v) {
    float kj, rj;
    if constexpr (kSpringPre) {
      kj = spring_k[0]; rj = spring_ref[0];
#pragma unroll
      for (int i = 1; i < kSpringN; ++i) { kj = j >= kWave * i ? spring_k[i] : kj; rj = j >= kWave * i ? spring_ref[i] : rj; }
    } else { kj = m.dof_stiffness[j]; rj = m.dof_springref[j]; }
    float passive = j < 6 ? 0.f : -kj * (s.qpos[j + 1] - rj) - dof_damp(s, m, j) * s.qvel[j];
    s.qfrc_smooth[j] = v + passive + s.vA[j];
  });
  STAGE(6);
  // ---- unconstrained acceleration
  // contact-space solve (nmf_dual.h) for steps with 1..kDualMaxCon contacts: the smooth solve keeps its factors for it
  bool dual = kDual<TP> && !WELD && ncon > 0 && ncon <= kDualMaxCon<TP> && !(m.solver_flags & 1);
  if constexpr (kDualH<TP>) dual = dual && __builtin_amdgcn_readfirstlane(s.body_cstart[TP::LB0] == s.body_cstart[1] ? 1 : 0) != 0;     // no contact on the rest of the body
  if constexpr (kDualGlob<TP>) dual = dual && m.noslip_iter == 0;      // (CPU flavour of ALL_POSSIBLE: primal loop + noslip_primal, see dual_solve)
  aba_solve<TP, WELD, !kDual<TP>>(s, V_QFRC_SMOOTH, V_QACC_SMOOTH, false, 0.f, m, lane, dual);
  contact_reload(c, s, lane);
  STAGE(7);

  // ---- constraint solve (Newton, exact line search) — mirrors oracle solve_constraints()
  int iters = 0;
  bool solved = false;
  unsigned int report = 0u;      // SolveReport bits
  float resid = 0.f;
  if constexpr (kDual<TP> && !WELD) {
    if (dual) {
      if (c.on) {      // reference accelerations of the rows: lane = row from here on
#pragma unroll
        for (int k = 0; k < 4; k++) dual_aref(s)[4 * lane + k] = c.aref[k];
      }
      WSYNC();
      // (CPU flavour: the noslip pass's acceleration is the step's qacc, s.qacc keeps the main solver's result — the warm start)
      float* const qout = m.noslip_iter > 0 && last ? st.qacc + (size_t)w * TP::NV : nullptr;
      iters = dual_solve<TP, kDualMaxCon<TP>>(s, m, lane, ncon, walls, report, resid, qout STAGE_PASS);
      solved = iters >= 0;       // (-1: rejected, the primal loop below solves the step)
      if (!solved) {             // the rows' reference accelerations come back from where the solve read them
        iters = 0; contact_reload(c, s, lane);
        if (c.on) {
#pragma unroll
          for (int k = 0; k < 4; k++) c.aref[k] = dual_aref(s)[4 * lane + k];
        }
      }
    }
  }
  if constexpr (kDual<TP>) { if (!solved && lane < kHistLds<TP>) s.act_hist[lane] = 0u; }      // nothing known for the next step
  // a step the contact-space solve cannot take has no noslip pass: counted (stats_sum column 13), never silent
  if (m.noslip_iter > 0 && !solved && ncon > 0) report |= kExitNoNoslip;
  if (!solved) report |= (ncon == 0 && !WELD) ? kExitFree : kExitPrimal;
  if (solved) {
  } else if (ncon == 0 && !WELD) {
    for (int j = lane; j < s.nv(); j += kWave) { s.qacc[j] = s.qacc_smooth[j]; s.vD[j] = 0.f; }
    WSYNC();
  } else {
    // The loop carries the gradient itself:  grad += alpha M search − JT (f_new − f_old)  after every move, one merged
    // leaf-to-root sweep (body wrenches alpha I_b T_b and the contact wrenches of −df together) instead of a product
    // with M plus a fresh JT f.  vA holds the Newton right-hand side −grad, vD the magnitude of the summed terms.
    float* Gv = s.vC; float* rhs = s.vA; float* search = s.vB; float* magv = s.vD;
    // Hybrid kernels, no rest body (head, abdomen, wings, ...) in contact: the cost depends on the rest's accelerations
    // through the Gauss term only, so they are minimised out in closed form.  What is left is the same problem over
    // root + legs with the rest's articulated inertia restA (from the factors of the smooth solve) added to the root
    // and the same unconstrained accelerations; the Newton loop below then never visits the rest's tree levels, and
    // the rest's accelerations follow from the root's at the end (one root-to-leaf pass over the cached factors).
    bool red = false;
    if constexpr (TP::kStar) { if constexpr (TP::REST_B > 0) {
      red = s.body_cstart[TP::LB0] == s.body_cstart[1];
      red = __builtin_amdgcn_readfirstlane(red ? 1 : 0) != 0;
      if (red) {       // (restA: left by the smooth solve, aba_solve)
        for (int j = lane; j < TP::NV; j += kWave) {
          const bool rest = j >= 6 && j < TP::LD0;
          search[j] = rest ? 0.f : s.qacc[j] - s.qacc_smooth[j];
          if (rest) { Gv[j] = 0.f; rhs[j] = 0.f; magv[j] = 0.f; }
        }
        if (lane == 0) s.reduced = 1;
        WSYNC();
      }
    } }
    // candidate 2 (the unconstrained acceleration) first: its body twists are what the smooth solve left in T
    float j0[4] = {0.f, 0.f, 0.f, 0.f}, w0 = 0.f, v0 = 0.f;
    if (c.on) { rows(ldsv(s.T[c.body]), j0);
#pragma unroll
      for (int k = 0; k < 4; k++) { j0[k] -= c.aref[k]; if (j0[k] < 0.f) v0 += 0.5f * c.D * j0[k] * j0[k]; } }
    if (wr.on) { w0 = s.T[0][wr.comp] - wr.aref; v0 += 0.5f * wr.D * w0 * w0; }
    WSYNC();
    // candidate 1: warm start
    float g = 0.f;
    if (red) {
      mul_M(s, search, m, lane, false, [&](int j, float v) {      // Gauss gradient M' (qacc − qacc_smooth)
        Gv[j] = v;
        g += 0.5f * search[j] * v;
      });
      if (c.on) rows(ldsv(s.T[c.body]), c.jar);  // J (qacc − qacc_smooth); candidate 2 adds J qacc_smooth − aref
      if (wr.on) wr.jar = s.T[0][wr.comp];
    } else {
      mul_M(s, s.qacc, m, lane, false, [&](int j, float v) {      // qacc still holds the warm start
        const float gv = v - s.qfrc_smooth[j];
        Gv[j] = gv;
        g += 0.5f * (s.qacc[j] - s.qacc_smooth[j]) * gv;
      });
      if (c.on) { rows(ldsv(s.T[c.body]), c.jar);
#pragma unroll
        for (int k = 0; k < 4; k++) c.jar[k] -= c.aref[k]; }
      if (wr.on) wr.jar = s.T[0][wr.comp] - wr.aref;
    }
    if (red) {
#pragma unroll
      for (int k = 0; k < 4; k++) c.jar[k] += j0[k];
      wr.jar += w0;
    }
    const float cost_ws_lane = constraint_cost_lane(c, wr);
    float gauss = wave_sum(g), ccost = wave_sum(cost_ws_lane);   // with the cost at the unconstrained acceleration: one round
    {
      const float cost_sm = wave_sum(v0);
      if (cost_sm < gauss + ccost) {
        gauss = 0.f; ccost = cost_sm;
        wr.jar = w0;
#pragma unroll
        for (int k = 0; k < 4; k++) c.jar[k] = j0[k];
        for (int j = lane; j < s.nv(); j += kWave) { s.qacc[j] = s.qacc_smooth[j]; Gv[j] = 0.f; }
      }
    }
    WSYNC();
    const float scale = 1.0f / (m.meaninertia * (float)s.nv());
    // gradient = (M qacc − qfrc_smooth) − JT f
    float gn = 0.f, gm = 0.f;
    {
      float f0[4] = {0.f, 0.f, 0.f, 0.f};
      if (c.on) contact_row_forces(c, -1.f, f0);
      contact_project<TP, false>(s, c, wr, fr, f0, wr.D * wr.jar, 0.f, m, lane, walls, [&](int j, float proj) {
        const float gv = Gv[j], qs = s.qfrc_smooth[j];
        const float gj = gv + proj;
        const float mag = fabsf(gv + qs) + fabsf(qs) + fabsf(proj);
        rhs[j] = -gj; magv[j] = mag;
        gn += gj * gj; gm += mag * mag;
      });
      gn = wave_sum(gn); gm = wave_sum(gm);
    }
    STAGE(8);
    for (int iter = 0; iter < m.max_iter; ++iter) {
      // converged, or the gradient is at its float32 rounding-noise floor (oracle: NMF_NOISE_FACTOR)
      if (scale * sqrtf(gn) < m.tolerance || sqrtf(gn) <= kNoiseFactor * 1.1920929e-07f * sqrtf(gm)) break;
      STAGE(9);
      aba_solve<TP, WELD>(s, V_A, V_B, true, 0.f, m, lane);   // search = −H⁻¹ grad ; T = twists(search)
      contact_reload(c, s, lane);
      STAGE(10);
      if (c.on) rows(ldsv(s.T[c.body]), c.jv);
      if (wr.on) wr.jv = s.T[0][wr.comp];
      // g1 = search·(M qacc − qfrc_smooth) = search·grad + (J search)·f ;  g2 = search·M·search as twice the kinetic
      // energy of the twists the ABA left in T (a sum of positive terms).  W keeps I_b T_b for the update sweep.
      float g1 = 0.f, g2 = 0.f;
      for_dofs(s, red, lane, [&](int j) { const float sj = search[j]; g1 -= sj * rhs[j]; g2 += s.arm[j] * sj * sj; });
      for_bodies(s, red, lane, [&](int b) {
        const SV tb = ldsv(s.T[b]);
        SV wb = inert_mul(s.Ib[b], tb);
        if constexpr (TP::kStar) { if constexpr (TP::REST_B > 0) { if (red && b == 0) wb = wb + rest_inertia_mul(s, tb); } }
        stsv(s.W[b], wb);
        g2 += dot(tb, wb);
      });
      // the rows' part of the line search's first evaluation (alpha = 0) rides the same reduction round as g1, g2: the
      // four wave sums interleave, and the search starts one dependent round later than it would otherwise
      float q1 = 0.f, q2 = 0.f;
      if (c.on) {
#pragma unroll
        for (int k = 0; k < 4; k++) if (c.jar[k] < 0.f) { q1 += c.D * c.jar[k] * c.jv[k]; q2 += c.D * c.jv[k] * c.jv[k]; }
      }
      if (wr.on) { q1 += wr.D * wr.jar * wr.jv; q2 += wr.D * wr.jv * wr.jv; }
      g1 -= q1;
      g1 = wave_sum(g1); g2 = wave_sum(g2);
      const float s1 = wave_sum(q1), s2 = wave_sum(q2);
      STAGE(11);
      // exact line search
      float alpha = 0.f, lo = 0.f, hi = -1.f;
      for (int ls = 0; ls < 30; ++ls) {
        float d1 = s1 + g1, d2 = s2 + g2;
        if (ls > 0) {
          d1 = 0.f; d2 = 0.f;
          if (c.on) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
              float x = c.jar[k] + alpha * c.jv[k];
              if (x < 0.f) { d1 += c.D * x * c.jv[k]; d2 += c.D * c.jv[k] * c.jv[k]; }
            }
          }
          if (wr.on) { const float x = wr.jar + alpha * wr.jv; d1 += wr.D * x * wr.jv; d2 += wr.D * wr.jv * wr.jv; }
          d1 = wave_sum(d1) + g1 + alpha * g2;
          d2 = wave_sum(d2) + g2;
        }
        if (d2 <= 0.f || d1 == 0.f) break;
        if (d1 < 0.f) lo = alpha; else hi = alpha;
        float next = alpha - d1 / d2;
        bool bisected = false;
        if (hi >= 0.f && (next <= lo || next >= hi)) { next = 0.5f * (lo + hi); bisected = true; }
        // phi' is linear while the active set does not change: then `next` is the exact minimiser
        bool moved = false;
        if (c.on) {
#pragma unroll
          for (int k = 0; k < 4; k++) moved |= ((c.jar[k] + alpha * c.jv[k]) < 0.f) != ((c.jar[k] + next * c.jv[k]) < 0.f);
        }
        const bool same = !bisected && !__any(moved);
        float change = fabsf(next - alpha);
        alpha = next;
        if (same || change <= 8.f * 1.1920929e-07f * fabsf(next)) break;
      }
      STAGE(12);
      if (alpha <= 0.f) break;
      // move:  qacc += alpha search;  grad += alpha M search − JT (f_new − f_old)
      float df[4] = {0.f, 0.f, 0.f, 0.f};
      if (c.on) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const float fo = c.jar[k] < 0.f ? c.D * c.jar[k] : 0.f;      // −f_old
          c.jar[k] += alpha * c.jv[k];
          df[k] = (c.jar[k] < 0.f ? c.D * c.jar[k] : 0.f) - fo;        // −(f_new − f_old)
        }
      }
      float dfw = 0.f;
      if (wr.on) { dfw = wr.D * alpha * wr.jv; wr.jar += alpha * wr.jv; }
      gn = 0.f; gm = 0.f;
      const float cost_lane = constraint_cost_lane(c, wr);     // of the moved residuals; summed with gn, gm below
      contact_project<TP, true>(s, c, wr, fr, df, dfw, alpha, m, lane, walls, [&](int j, float x) {
        const float sj = search[j];
        x += alpha * s.arm[j] * sj;
        s.qacc[j] += alpha * sj;
        const float r = rhs[j] - x, mag = magv[j] + fabsf(x);
        rhs[j] = r; magv[j] = mag;
        gn += r * r; gm += mag * mag;
      });
      gn = wave_sum(gn); gm = wave_sum(gm);
      const float newccost = wave_sum(cost_lane);              // one reduction round for the three
      // the Gauss term is quadratic along the search direction: its change is exact from g1, g2
      const float dgauss = alpha * (g1 + 0.5f * alpha * g2);
      iters = iter + 1;
      STAGE(13);
      const float improvement = (ccost - newccost) - dgauss;
      gauss += dgauss; ccost = newccost;
      // (the rounding-floor test on the improvement: a guard against cycling from the ninth iteration on — see nmf_dual.h)
      if (scale * improvement < m.tolerance || (iter >= 8 && improvement <= kNoiseFactor * 1.1920929e-07f * fabsf(gauss + ccost))) break;
    }
    STAGE(9);
    // constraint forces
    {
      float ff[4] = {0.f, 0.f, 0.f, 0.f};
      if (c.on) contact_row_forces(c, 1.f, ff);
      contact_project<TP, false>(s, c, wr, fr, ff, -wr.D * wr.jar, 0.f, m, lane, walls, [&](int j, float v) { s.vD[j] = v; });
    }   // qfrc_constraint lives in vD until the Euler step
    if constexpr (TP::kStar) { if constexpr (TP::REST_B > 0) {
      if (red) {     // the rest's accelerations: qacc_smooth + the response of the cached factors to the root's change
        if (lane < 6) {
          float tw = 0.f;
#pragma unroll
          for (int j = 0; j < 6; ++j) tw += (s.qacc[j] - s.qacc_smooth[j]) * s.S[j][lane];
          s.T[0][lane] = tw;
        }
        if (lane == 0) s.reduced = 0;
        WSYNC();
        const LaneRole L = lane_role<TP>(lane);
        if (m.rest_fast) rest_levels<TP, true, false>(s, lane, [&](const auto& nd) { rest_aba_expand<TP, 3, true>(s, nd, s.qacc, L); });
        else rest_levels<TP, false, false>(s, lane, [&](const auto& nd) { rest_aba_expand<TP, 0, true>(s, nd, s.qacc, L); });
      }
    } }
    // ---- CPU flavour: the noslip post-pass (noslip_primal), then J^T f and qacc = M^-1 (qfrc_smooth + J^T f) from its forces
    if (nsbuf && ncon > 0) {
      float f0[4] = {0.f, 0.f, 0.f, 0.f};
      if (c.on) contact_row_forces(c, 1.f, f0);
      WSYNC();
      noslip_primal<TP, WELD>(s, m, lane, nsbuf, ncon, walls, c.on, c.info, f0[0], f0[1], f0[2], f0[3], -wr.D * wr.jar, wr.D);
      contact_reload(c, s, lane);
      float ff[4] = {0.f, 0.f, 0.f, 0.f};
      if (c.on) {
#pragma unroll
        for (int k = 0; k < 4; k++) ff[k] = nsbuf[kNoslipRows * kNoslipRows + kNoslipRows + 4 * opaque(lane) + k];
      }
      contact_project<TP, false>(s, c, wr, fr, ff, -wr.D * wr.jar, 0.f, m, lane, walls, [&](int j, float v) { s.vD[j] = v; s.vA[j] = s.qfrc_smooth[j] + v; });
      // (into vB: qacc keeps the main solver's result, which is the next step's warm start — MuJoCo saves it before its noslip
      // pass, mj_fwdConstraint; the acceleration with the noslip forces is a pure output of the launch's last step)
      aba_solve<TP, WELD>(s, V_A, V_B, false, 0.f, m, lane);
      contact_reload(c, s, lane);
      if (last) { for (int j = lane; j < s.nv(); j += kWave) st.qacc[(size_t)w * s.nv() + opaque(j)] = s.vB[j]; }
      report &= ~kExitNoNoslip;
    }
  }
  if (lane == 0) { s.iters = (int)((unsigned int)iters | report); s.solve_resid = resid; }
  STAGE(14);

  // ---- contact sensors (oracle contact_sensors): a pure output, evaluated on the launch's last step (into the batch's arrays)
  // and on the steps an observation ring records (into the ring's row), written straight to HBM.  c_w holds the world-frame
  // contact wrenches about the root origin.
  if (last) {
    const int ol = opaque(lane);
    if (lane < kMaxCon) st.contact_geom[(size_t)w * kMaxCon + ol] = c.on ? (float)info_geom(c.info) : -1.f;
  }
  // the contacts of every leg sensor as a bit mask: lane = contact tells its sensor, lane s < 6 keeps sensor s's mask and walks
  // its own one or two contacts (in contact order: the sums are those of a walk over the whole list) instead of all of them
  unsigned long long smask = 0ull;
  if (last || rec) {
    const int my_s = lane < ncon ? info_sensor(s.c_info[lane]) : -1;
#pragma unroll
    for (int q = 0; q < 6; ++q) { const unsigned long long bq = __ballot(my_s == q); smask = lane == q ? bq : smask; }
  }
  for (int dest = 0; dest < 2; ++dest) {
    float* out = dest == 0 ? (last ? &st.sensordata[(size_t)w * 96] : nullptr) : (rec ? rec + 2 * st.ring_nj + st.ring_nact : nullptr);
    if (!out) continue;
    const int ol = opaque(lane);
    for (int i = ol; i < 96; i += kWave) out[i] = 0.f;
    WSYNC();
    if (m.nsensor && lane < 6 && smask) {
      float wsum = 0.f; V3 pc = v3(0, 0, 0), pm = v3(0, 0, 0), F = v3(0, 0, 0), Tq = v3(0, 0, 0); int cnt = 0;
      Frame f1 = fr;                       // frame of the leg's first contact (what the sensor reports as normal / tangent)
      for (unsigned long long mk = smask; mk; mk &= mk - 1ull) {
        const int cc = __ffsll((long long)mk) - 1;
        V3 f = ld3(&s.c_w[cc][3]);
        const Frame cf = walls ? contact_frame(info_fid(s.c_info[cc]), fr) : fr;
        if (cnt == 0) f1 = cf;
        float fn = dot(f, cf.n);
        V3 p = ld3(s.c_r[cc]);
        wsum += fn; pc = pc + fn * p; pm = pm + p; cnt++;
      }
      pc = wsum > 0.f ? (1.0f / wsum) * pc : (1.0f / (float)cnt) * pm;
      for (unsigned long long mk = smask; mk; mk &= mk - 1ull) {
        const int cc = __ffsll((long long)mk) - 1;
        V3 f = ld3(&s.c_w[cc][3]);
        F = F + f;
        Tq = Tq + cross(ld3(s.c_r[cc]) - pc, f);
      }
      float* o16 = out + 16 * ol;
      V3 o = ld3(s.xpos()[0]);
      if (m.sem_sensor_contact_frame) {    // net force / torque expressed in the contact frame (normal, t1, t2)
        F = v3(dot(f1.n, F), dot(f1.t1, F), dot(f1.t2, F));
        Tq = v3(dot(f1.n, Tq), dot(f1.t1, Tq), dot(f1.t2, Tq));
      }
      o16[0] = (float)cnt; st3(o16 + 1, F); st3(o16 + 4, Tq); st3(o16 + 7, pc + o); st3(o16 + 10, f1.n); st3(o16 + 13, f1.t1);
    }
  }
  WSYNC();
  STAGE(17);
  return solved;     // the constraint forces are contact wrenches in c_w (contact-space solve), not J^T f in vD
}

template <class TP, bool WELD>
__device__ void physics_integrate(FlyLds<TP>& s, const GModel& m, int lane, bool wrenches STAGE_ARG) {
  // (per-lane addresses of this stage are rebuilt every step where the allocator otherwise parks them in scratch from the
  // kernel's prologue on: the hybrid kernels and the leg-chain terrain kernels, 11 reloads per step each a memory round trip)
  if constexpr (TP::kStar) { if constexpr (TP::REST_B > 0 || TP::kTerrain) lane = opaque(lane); }
  const Frame fr = make_frame(v3(m.plane[0], m.plane[1], m.plane[2]));
  const float h = m.timestep;
  wrenches = __builtin_amdgcn_readfirstlane((int)wrenches) != 0;
  if (wrenches) {
    if constexpr (kDualH<TP>) {      // (see dual_wrench)
      if (lane < s.ncon) {
#pragma unroll
        for (int i = 0; i < 6; ++i) dual_wrench(s)[lane][i] = s.c_w[lane][i];
      }
      WSYNC();
    }
    aba_solve<TP, WELD, !kDual<TP>>(s, V_QFRC_SMOOTH, V_B, false, h, m, lane, false, true);
  }
  else {
    for (int j = lane; j < s.nv(); j += kWave) s.vA[j] = s.qfrc_smooth[j] + s.vD[j];
    WSYNC();
    aba_solve<TP, WELD, !kDual<TP>>(s, V_A, V_B, false, h, m, lane);
  }
  // Semi-implicit Euler in one pass: qvel += h a, then positions with the NEW velocities — a hinge's own (the same lane holds
  // it), the root's from lanes 0..5 through scalar registers (no second trip through LDS, no lane working alone while 63 wait:
  // every lane computes the root's quaternion from the same scalars, lane 0 stores it).  Two turns of the wave (72 dofs) read
  // both turns' operands before the first turn's stores.
  const Q4 q0 = ldq(&s.qpos[3]);
  float v0 = 0.f;      // the first turn's new velocity: lanes 0..5 hold the root's
  if constexpr (TP::kStar) {
    if constexpr (TP::NV > kWave && TP::NV <= 2 * kWave) {
      const int jb = lane + kWave;
      const bool two = jb < TP::NV;
      const float va = s.qvel[lane] + h * s.vB[lane];
      const float pa = lane >= 6 ? s.qpos[lane + 1] : 0.f;
      float vb2 = 0.f, pb = 0.f;
      if (two) { vb2 = s.qvel[jb] + h * s.vB[jb]; pb = s.qpos[jb + 1]; }
      s.qvel[lane] = va;
      if (lane >= 6) s.qpos[lane + 1] = pa + h * va;
      if (two) { s.qvel[jb] = vb2; s.qpos[jb + 1] = pb + h * vb2; }
      v0 = va;
    }
  }
  if (!(TP::kStar && TP::NV > kWave && TP::NV <= 2 * kWave)) {
    for (int j = lane; j < s.nv(); j += kWave) {
      const float v = s.qvel[j] + h * s.vB[j];
      s.qvel[j] = v;
      if (j >= 6) s.qpos[j + 1] += h * v;
      if (j < kWave) v0 = v;
    }
  }
  {
    const V3 w = v3(readlane_f(v0, 3), readlane_f(v0, 4), readlane_f(v0, 5));
    if (lane < 3) s.qpos[lane] += h * v0;
    const float wn = sqrtf(dot(w, w));
    Q4 q = q0;
    if (wn > kMinVal) {
      float sn, cs;
      sincos_bounded(0.5f * h * wn, &sn, &cs);
      V3 ax = (sn / wn) * w;
      q = qmul(q, Q4{cs, ax.x, ax.y, ax.z});
    }
    q = qnorm(q);
    if (lane == 0) stq(&s.qpos[3], q);
  }
  WSYNC();
}

// The state a world carries from one workgroup to the next inside a chunked launch (qpos, qvel, warm start, controls,
// clock, running sums) crosses HBM with agent-scope accesses: such loads / stores bypass the caches that are not
// coherent between XCDs, so the hand-off needs no L2 write-back / invalidate fence (which costs tens of microseconds
// with every wave of the chip fencing) — only "stores done before the flag", i.e. s_waitcnt vmcnt(0).
__device__ __forceinline__ float ld_state(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_state(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// *p += v at agent scope, result not needed (global_atomic_add_f32 without return: no round trip to wait for)
__device__ __forceinline__ void add_state(float* p, float v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void add_count(unsigned int* p, unsigned int v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Hand-off between two chunks of a launch: DATA-TAGGED GRANULES.  Every float of the state travels as one 8-byte word
// {float bits, tag} written and read with ONE 64-bit relaxed agent-scope atomic (global_store / global_load_dwordx2 sc1:
// single-copy atomic by the memory model, never torn, never served from a non-coherent cache).  The tag names the
// launch and the number of chunks the world has finished, so a granule is valid exactly when its tag is the one the
// reader expects — each granule on its own.  No flag, hence no "all stores done before the flag" drain on the writer
// (it goes straight on to its next item) and no flag round trip before the state loads on the reader: one batch of loads,
// re-issued only if a tag is still old.  (Round 2 handed over through the state arrays + a per-world flag: writer
// s_waitcnt vmcnt(0) -> flag store; reader flag poll -> state loads — ~12 us per item against ~5 us now.)
__device__ __forceinline__ void st_tagged(unsigned long long* p, float v, unsigned int tag) {
  __hip_atomic_store(p, ((unsigned long long)tag << 32) | (unsigned long long)__float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float ld_tagged(const unsigned long long* p, unsigned int want, bool& ok) {
  const unsigned long long g = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  ok = ok && (unsigned int)(g >> 32) == want;
  return __uint_as_float((unsigned int)g);
}
// the same granules carrying raw 32-bit payloads (counters, bit masks): never through a float register
__device__ __forceinline__ void st_tagged_u(unsigned long long* p, unsigned int v, unsigned int tag) {
  __hip_atomic_store(p, ((unsigned long long)tag << 32) | (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned int ld_tagged_u(const unsigned long long* p, unsigned int want, bool& ok) {
  const unsigned long long g = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  ok = ok && (unsigned int)(g >> 32) == want;
  return (unsigned int)g;
}

// `final`: this item ends the launch.  Pure outputs (plain stores: qacc, stats — like the pose / sensor / force outputs of
// the last step) are written by the final item only: an earlier chunk's plain store, sitting in another XCD's L2, could
// otherwise reach memory after the final one's.
template <class TP>
__device__ void write_outputs(FlyLds<TP>& s, const GModel& m, const DevState& st, int w, int lane, float time, bool final,
                              unsigned int tag = 0u, unsigned int carry = 0u) {
  lane = opaque(lane);     // once per item: keep its address arithmetic out of the registers the steps live in
  if (!final) {            // an inner chunk of a chunked launch: the state goes to the world's next item as tagged granules
    unsigned long long* hb = st.handoff + (size_t)w * st.handoff_stride;
    const int nq = s.nq(), nv = s.nv();
    for (int i = lane; i < nq; i += kWave) st_tagged(&hb[i], s.qpos[i], tag);
    for (int i = lane; i < nv; i += kWave) { st_tagged(&hb[nq + i], s.qvel[i], tag); st_tagged(&hb[nq + nv + i], s.qacc[i], tag); }
    for (int i = lane; i < m.nu; i += kWave) st_tagged(&hb[nq + 2 * nv + i], s.ctrl[i], tag);
    // lanes 0..5: the clock (float bits) and what the world's items have accumulated so far (steps, contacts, iterations,
    // overflow steps: unsigned integers; cycles: float bits): one store; the launch's final item adds them to the world's counters
    if (lane < 6) st_tagged_u(&hb[nq + 2 * nv + m.nu + lane], lane == 0 ? __float_as_uint(time) : carry, tag);
    if constexpr (kDual<TP>) { if (lane < hist_words<TP>(m)) st_tagged_u(&hb[nq + 2 * nv + m.nu + 6 + lane], s.act_hist[lane], tag); }
    return;
  }
  if constexpr (kDual<TP>) { if (lane < kActHistWords) st.act_hist[(size_t)w * kActHistWords + lane] = lane < hist_words<TP>(m) ? s.act_hist[lane < kHistLds<TP> ? lane : 0] : 0u; }
  // CPU flavour, last step in contact and solved by the primal loop: its noslip pass has written the step's acceleration itself
  // (s.qacc is the warm start)
  const bool noslip_qacc = m.noslip_iter > 0 && st.noslip_buf && s.ncon > 0 && ((unsigned int)s.iters & (kExitPrimal | kExitDual)) != 0u;
  for (int i = lane; i < s.nq(); i += kWave) st_state(&st.qpos[(size_t)w * s.nq() + i], s.qpos[i]);
  for (int i = lane; i < s.nv(); i += kWave) {
    st_state(&st.qvel[(size_t)w * s.nv() + i], s.qvel[i]);
    st_state(&st.qacc_ws[(size_t)w * s.nv() + i], s.qacc[i]);
    if (final && !noslip_qacc) st.qacc[(size_t)w * s.nv() + i] = s.qacc[i];
  }
  for (int i = lane; i < m.nu; i += kWave) {
    st_state(&st.ctrl[(size_t)w * m.nu + i], s.ctrl[i]);
  }
  if (lane == 0) st_state(&st.time[opaque(w)], time);      // (opaque: the address is not kept in a register pair from the item's start)
  if (lane == 0 && final) {
    float* q = &st.stats[8 * (size_t)w];
    q[0] = (float)s.ncon; q[1] = (float)(s.iters & 0xff); q[2] = (float)s.overflow; q[3] = (float)(4 * s.ncon);
    q[4] = (float)((s.iters >> 8) & 0xfff); q[5] = (float)((s.iters >> 20) & 0x7f); q[6] = s.solve_resid; q[7] = 0.f;
  }
}

// Pose outputs (named segments, sites) of the poses the last kinematics stage computed.  Called while the body poses
// are alive in LDS: right after the collision stage of a launch's last step (as in the reference engine, the poses a
// step reports belong to the state before its integration), or after the kinematics of a reset.
template <class TP>
__device__ void write_poses(FlyLds<TP>& s, const GModel& m, const DevState& st, int w, int lane) {
  lane = opaque(lane);     // once per launch (see write_outputs)
  for (int sg = lane; sg < m.nseg; sg += kWave) {
    int b = m.seg_body[sg];
    V3 p = ld3(s.xpos()[b]) + mat_vec(s.xmat()[b], ld3(&m.seg_pos[3 * sg]));
    Q4 q = qnorm(qmul(mat_quat(s.xmat()[b]), ldq(&m.seg_quat[4 * sg])));
    if (q.w < 0.f) q = Q4{-q.w, -q.x, -q.y, -q.z};
    st3(&st.seg_xpos[((size_t)w * m.nseg + sg) * 3], p);
    stq(&st.seg_xquat[((size_t)w * m.nseg + sg) * 4], q);
  }
  for (int sg = lane; sg < m.nsite; sg += kWave) {
    int b = m.site_body[sg];
    V3 p = ld3(s.xpos()[b]) + mat_vec(s.xmat()[b], ld3(&m.site_pos[3 * sg]));
    st3(&st.site_xpos[((size_t)w * m.nsite + sg) * 3], p);
  }
}

// Waves per SIMD the register allocation aims at: two (256 VGPRs).  Three (168 VGPRs) were measured on both leg-chain
// skeletons: the 72-dof kernel gains nothing (the LDS array saturates), the
// 48-dof one +18 % with 70 spilled registers in an early round-2 build but -12 % with the 116 the persistent item loop
// leaves it — not shipped.
template <class TP> constexpr int waves_per_simd() { return 2; }

// What every kernel of a batch stages in LDS once per launch: the tree tables (kernels with tree sweeps), the per-dof
// diagonal terms, the per-row constants of the contact stiffness rows / inertia rows, and — star kernels with LDS to spare —
// the part of the model the non-inlined stages read (HotModel), the contact frame and the joint axes.
template <class TP>
__device__ __forceinline__ void stage_launch_constants(FlyLds<TP>& s, const GModel& m) {
  if constexpr (!TP::kStar) { if (threadIdx.x == 0) { s.rt_nb = m.nb; s.rt_nv = m.nv; } __syncthreads(); }
  if constexpr (TP::kNFact > 1) {     // kernels with tree sweeps: stage the tree tables
    for (int b = threadIdx.x; b < TP::kTblB && b < m.nb; b += kWave) {
      s.t_body[b] = (unsigned char)m.tree_body[b < m.tree_lvl_start[m.tree_nlevel] ? b : 0];
      s.t_parent[b] = (unsigned char)(b ? m.body_parent[b] : 0);
      s.t_dofadr[b] = (unsigned char)m.body_dofadr[b]; s.t_dofnum[b] = (unsigned char)m.body_dofnum[b];
      s.t_cstart[b] = (unsigned char)m.tree_child_start[b]; s.t_ccount[b] = (unsigned char)m.tree_child_count[b];
    }
    for (int j = threadIdx.x; j < TP::kTblV && j < m.nv; j += kWave) s.t_dofbody[j] = (unsigned char)m.dof_body[j];
    if (threadIdx.x < 18) s.t_lvl[threadIdx.x] = (unsigned char)m.tree_lvl_start[threadIdx.x];
    if (threadIdx.x == 0) s.t_nlevel = (unsigned char)m.tree_nlevel;
    if constexpr (TP::kStar) {
      for (int i = threadIdx.x; i < kRestLevels * 16; i += kWave) (&s.t_pack[0][0][0])[i] = m.rest_fast ? m.rest_pack[i] : 0xffffffffu;
    }
    __syncthreads();
  }
  const int lane = threadIdx.x;
  for (int j = lane; j < s.nv(); j += kWave) {
    if constexpr (row_width_s<TP>() > 6) s.S[j][6] = 0.f;      // padding column: the shadow rows' axis component (aba_solve)
    s.arm[j] = m.dof_armature[j];
    if constexpr (kHasCm3<TP>) { s.damp[j] = m.dof_damping[j]; s.dlt[j] = m.dof_armature[j] + m.timestep * m.dof_damping[j]; }
  }
  if (lane < 6) {
    const KLane K = k_lane(lane, make_frame(v3(m.plane[0], m.plane[1], m.plane[2])));
    float* q = s.k_tab[lane];
#pragma unroll
    for (int i = 0; i < 3; ++i) { q[i] = K.dA[i]; q[3 + i] = K.dB[i]; q[6 + i] = K.dO[i]; }
    q[9] = __int_as_float(K.ia); q[10] = __int_as_float(K.ib);
    int words[3];
    inertia_map_pack(lane, words);
    q[11] = __int_as_float(words[0]); q[12] = __int_as_float(words[1]); q[13] = __int_as_float(words[2]);
    if constexpr (kHasIsym<TP>) {
#pragma unroll
      for (int c = 0; c < 6; c++) {
        const int i = lane < c ? lane : c, jx = lane < c ? c : lane;
        q[14 + c] = __int_as_float(i * 6 - i * (i - 1) / 2 + (jx - i));
      }
    }
  }
  if constexpr (kHasIsym<TP>) if (lane == 0) {
    const Frame fr = make_frame(v3(m.plane[0], m.plane[1], m.plane[2]));
    st3(&s.frame9[0], fr.n); st3(&s.frame9[3], fr.t1); st3(&s.frame9[6], fr.t2);
    HotModel& h = s.hot;
    h.dof_axis = m.dof_axis; h.body_pos = m.body_pos; h.body_quat = m.body_quat; h.geom_p0 = m.geom_p0; h.geom_p1 = m.geom_p1;
    h.geom_radius = m.geom_radius; h.geom_bsphere = m.geom_bsphere; h.hull_vert = m.hull_vert; h.pair_margin = m.pair_margin;
    h.geom_body = m.geom_body; h.geom_type = m.geom_type; h.geom_hulladr = m.geom_hulladr; h.geom_hullnum = m.geom_hullnum;
#pragma unroll
    for (int i = 0; i < 4; ++i) h.plane[i] = m.plane[i];
#pragma unroll
    for (int i = 0; i < 5; ++i) h.terrain[i] = m.terrain[i];
    h.hull_skin = m.hull_skin; h.terrain_type = m.terrain_type; h.ng = m.ng; h.sem_max_hull_contacts = m.sem_max_hull_contacts;
    h.terrain_walls = m.sem_terrain_walls;
  }
  if constexpr (kHasIsym<TP>) for (int i = lane; i < 3 * s.nv(); i += kWave) (&s.axis[0][0])[i] = m.dof_axis[i];
}

// Reset to the keyframe and refresh the pose outputs (no stepping): one workgroup per world; reset_mask (may be null)
// selects the worlds.  Its own kernel: inside the stepping kernel the reset path's addresses and constants were hoisted out
// of the persistent item loop and held (or spilled) across every step.
template <class TP>
__global__ void __launch_bounds__(kWave) nmf_reset_kernel(const DevModel* __restrict__ mp, DevState st, const unsigned char* __restrict__ reset_mask) {
  __shared__ FlyLds<TP> s;
  const GModel& m = *(const GModel*)mp;
  const int lane = threadIdx.x, w = (int)blockIdx.x;
  if (w >= st.n_worlds || (reset_mask && !reset_mask[w])) return;
  stage_launch_constants(s, m);
  for (int i = lane; i < s.nq(); i += kWave) s.qpos[i] = m.key_qpos[i];
  for (int i = lane; i < s.nv(); i += kWave) { s.qvel[i] = 0.f; s.qacc[i] = 0.f; }
  for (int i = lane; i < m.nu; i += kWave) { s.ctrl[i] = m.key_ctrl[i]; st.actuator_force[(size_t)w * m.nu + i] = 0.f; st.act[(size_t)w * m.nu + i] = 0.f; }
  for (int i = lane; i < 96; i += kWave) st.sensordata[(size_t)w * 96 + i] = 0.f;
  if (lane == 0) { s.ncon = 0; s.iters = 0; s.overflow = 0; s.solve_resid = 0.f; }
  WSYNC();
  stage_kinematics(s, m, lane);
  write_poses(s, m, st, w, lane);
  write_outputs(s, m, st, w, lane, 0.f, true);
  if (lane < 16) st.stats_sum[16 * (size_t)w + lane] = 0u;
  if (lane < kActHistWords) st.act_hist[(size_t)w * kActHistWords + lane] = 0u;
  if (lane < kMaxCon) st.contact_geom[(size_t)w * kMaxCon + lane] = -1.f;
}

// Step n_steps times.  Which world, which steps — two schedules (DevState::sched_mode):
//   plain   (0): workgroup b steps world order[b] through all n_steps and exits (every world resident at once).
//   chunked (1): more worlds than resident waves.  The launch is cut into n_chunks chunks (long first, short last), the
//     grid is one PERSISTENT workgroup per resident wave, and each takes (chunk, world) items from a ticket counter until
//     the counter runs out: ticket t = (chunk t / n_worlds, world order[t % n_worlds]).  A world's cost varies 2x with its
//     gait phase (and by +-30 % from one 20-step launch to the next: contact events), so whole-launch items leave the
//     machine half empty while the costliest worlds finish; with chunks the tail is one chunk long.  An item's state
//     comes from the world's previous chunk — an older ticket, hence taken by a workgroup that is running or done: no
//     deadlock whatever the dispatch order — as data-tagged granules (st_tagged / ld_tagged).
//   (Measured and dropped, round 3: a static cost-balanced partition — persistent workgroups stepping the worlds of ranks
//    b, 2R-1-b, ... of the cost order through the whole launch, no hand-over at all.  A world's cost predicts its next
//    launch's only to r = 0.88, and the costliest world takes 1.6x the mean: the costliest-with-cheapest pair sums spread
//    to 1.30x their mean, 35.9 M env-steps/s against 42.4 M chunked on 20-step launches.)
// The model constants staged above stay in LDS from item to item.  Worlds are independent: the schedule never changes a result.
template <class TP, bool WELD>
__global__ void __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(waves_per_simd<TP>(), waves_per_simd<TP>()))) nmf_step_kernel(const DevModel* __restrict__ mp, DevState st, ReplayArgs rp, int n_steps) {
  __shared__ FlyLds<TP> s;
  const GModel& m = *(const GModel*)mp;      // the model lives in HBM: its fields load as global memory in every function
  const unsigned long long probe_c0 = __builtin_amdgcn_s_memtime(), probe_r0 = __builtin_amdgcn_s_memrealtime();
  TRACE_DECL();
  const int lane = threadIdx.x;
  const bool chunked = st.sched_mode == 1;
  // the first ticket is requested before the launch constants are staged: its round trip hides behind them
  unsigned int t_first = 0;
  if (chunked && lane == 0) t_first = atomicAdd(&st.csched->ticket, 1u);
  stage_launch_constants(s, m);
  if constexpr (kDualGlob<TP>) { if (lane == 0) s.dual_glob[0] = st.dual_scratch + (size_t)blockIdx.x * kDualScratchFloats; }
  unsigned int t_next = (unsigned int)__builtin_amdgcn_readfirstlane((int)t_first);
  STAGE_INIT();
  const int n_chunks = chunked ? st.n_chunks : 1;
  const unsigned int epoch = chunked ? (unsigned int)__builtin_amdgcn_readfirstlane((int)st.csched->epoch) : 0u;
  for (;;) {
    int slot = (int)blockIdx.x, chunk = 0, step0 = 0, step1 = n_steps;
    if (chunked) {
      const unsigned int t = t_next;
      if (t >= (unsigned int)st.n_worlds * (unsigned int)n_chunks) {
        // out of items.  The last workgroup to get here rewinds the counters for the next launch (no host-side state,
        // so hipGraph replays stay valid); every workgroup has taken its final ticket by then.
        if (lane == 0 && atomicAdd(&st.csched->exited, 1u) == gridDim.x - 1u) {
          st.csched->ticket = 0u; st.csched->exited = 0u; st.csched->epoch = epoch + 1u;
        }
        break;
      }
      chunk = (int)(t / (unsigned int)st.n_worlds); slot = (int)(t % (unsigned int)st.n_worlds);
      step0 = st.chunk_start[chunk]; step1 = st.chunk_start[chunk + 1];
    } else if (slot >= st.n_worlds) return;
    const int w = __builtin_amdgcn_readfirstlane(st.order ? st.order[slot] : slot);     // wave-uniform: lives in a scalar register
    TRACE_SUB(2);
    const unsigned long long t_begin = __builtin_amdgcn_s_memtime();
    if (st.sched && lane == 0) atomicMin(&st.sched->t_first, (unsigned long long)__builtin_amdgcn_s_memrealtime());
    float time;
    unsigned int carry = 0u; // lanes 1..4: what the world's earlier items of this launch accumulated (steps, contacts, iterations, overflow steps); lane 5: their cycles (float bits)
    unsigned int sum_con = 0u, sum_it = 0u, sum_of = 0u;     // running sums over the steps of this item (wave-uniform)
    unsigned int sum_dual = 0u, sum_kkt = 0u;                // ... steps solved in contact space / ended on the KKT test (scalar registers)
    {
      // control table: lane a < 64 carries column a; the row of step s + 1 is requested while step s runs, so its
      // HBM latency (~1.5 k cycles per step when loaded on demand) is off the step's critical path; the item's first
      // row travels with the state
      const float* tab = rp.table ? rp.table + (size_t)w * rp.table_steps * rp.n_act : nullptr;
      const int ln = opaque(lane);      // once per item (see write_outputs)
      const int my_ctrl = tab && lane < rp.n_act ? rp.act_ids[ln] : -1;
      CtrlPrefetch pf;
      pf.mine = my_ctrl >= 0; pf.next_row = nullptr;
      pf.value = my_ctrl >= 0 ? tab[(size_t)((rp.start + step0) % rp.table_steps) * rp.n_act + lane] : 0.f;     // the item's first row travels with the state
      if (chunk > 0) {
        // the world's previous chunk (an older ticket: its item is running or done) leaves the state as tagged granules
        const unsigned int want = (unsigned int)__builtin_amdgcn_readfirstlane((int)(epoch * 32u + (unsigned int)chunk));
        const unsigned long long* hb = st.handoff + (size_t)w * st.handoff_stride;
        const int nq = s.nq(), nv = s.nv();
        for (;;) {
          bool ok = true;
          for (int i = ln; i < nq; i += kWave) s.qpos[i] = ld_tagged(&hb[i], want, ok);
          for (int i = ln; i < nv; i += kWave) { s.qvel[i] = ld_tagged(&hb[nq + i], want, ok); s.qacc[i] = ld_tagged(&hb[nq + nv + i], want, ok); }
          for (int i = ln; i < m.nu; i += kWave) s.ctrl[i] = ld_tagged(&hb[nq + 2 * nv + i], want, ok);
          carry = lane < 6 ? ld_tagged_u(&hb[nq + 2 * nv + m.nu + ln], want, ok) : 0u;     // lane 0: the clock; 1..5: running sums
          if constexpr (kDual<TP>) { const unsigned int hw = lane < hist_words<TP>(m) ? ld_tagged_u(&hb[nq + 2 * nv + m.nu + 6 + ln], want, ok) : 0u; if (lane < kHistLds<TP>) s.act_hist[lane] = hw; }
          if (!__any(!ok)) break;            // wave-uniform: every granule carried the expected tag
          __builtin_amdgcn_s_sleep(8);
        }
        time = __uint_as_float((unsigned int)__builtin_amdgcn_readlane((int)carry, 0));
      } else {
        for (int i = ln; i < s.nq(); i += kWave) s.qpos[i] = ld_state(&st.qpos[(size_t)w * s.nq() + i]);
        for (int i = ln; i < s.nv(); i += kWave) {
          s.qvel[i] = ld_state(&st.qvel[(size_t)w * s.nv() + i]);
          s.qacc[i] = ld_state(&st.qacc_ws[(size_t)w * s.nv() + i]);
        }
        for (int i = ln; i < m.nu; i += kWave) s.ctrl[i] = ld_state(&st.ctrl[(size_t)w * m.nu + i]);
        if constexpr (kDual<TP>) { if (lane < kHistLds<TP>) s.act_hist[lane] = st.act_hist[(size_t)w * kActHistWords + ln]; }
        time = ld_state(&st.time[w]);
      }
      WSYNC();
      TRACE_GAP_END();
      for (int step = step0; step < step1; ++step) {
        if (tab) {
          if (my_ctrl >= 0) s.ctrl[my_ctrl] = pf.value;
          const float* src = tab + (size_t)((rp.start + step) % rp.table_steps) * rp.n_act;
          for (int a = opaque(lane) + kWave; a < rp.n_act; a += kWave) s.ctrl[rp.act_ids[a]] = src[a];     // (more than 64 controls: hybrid / tree kernels)
          pf.next_row = step + 1 < step1 ? tab + (size_t)((rp.start + step + 1) % rp.table_steps) * rp.n_act : nullptr;
          WSYNC();
        }
        STAGE(0);
        // an observation ring records this step: its row (wave-uniform address)
        float* rec = nullptr;
        if (st.obs_every > 0 && (step + 1) % st.obs_every == 0)
          rec = st.ring + ((size_t)((step + 1) / st.obs_every - 1) * (size_t)st.n_worlds + (size_t)w) * (size_t)st.ring_stride;
        const bool wrenches = physics_forward<TP, WELD>(s, m, lane, st, w, step == n_steps - 1, rec, pf STAGE_PASS);     // pure outputs: the launch's last step and the recorded ones
        physics_integrate<TP, WELD>(s, m, lane, wrenches STAGE_PASS);
        if (rec) {       // the state after the step, as nmf_pack_observations reads it after a launch
          const int nj = st.ring_nj;
          for (int i = opaque(lane); i < nj; i += kWave) { rec[i] = s.qpos[7 + i]; rec[nj + i] = s.qvel[6 + i]; }
        }
        STAGE(15);
        time += m.timestep;
        // how the step's solve ended.  The two common kinds (solved in contact space, ended on the KKT test) are counted in scalar
        // registers and added once per item; any other bit of the report — one step in ten thousand — goes straight to the world's
        // counter from lane 6 + k, an atomic the wave does not wait for
        const unsigned int rep = (unsigned int)__builtin_amdgcn_readfirstlane(s.iters);
        sum_con += (unsigned int)s.ncon; sum_it += rep & 0xffu; sum_of += (unsigned int)s.overflow;
        sum_dual += (rep >> 8) & 1u; sum_kkt += (rep >> 9) & 1u;
        if (rep & (0xffcu << 8)) {
          const int xl = opaque(lane) - 6;
          if (xl >= 2 && xl < kExitKinds && ((rep >> (8 + xl)) & 1u)) add_count(&st.stats_sum[16 * (size_t)w + 4 + xl], 1u);
        }
      }
    }
    TRACE_BUSY_END();
    TRACE_SUB_RESET();
    // the next item's ticket BEFORE this item's state goes out: a wave's memory operations complete in order, so a ticket
    // requested behind the write-through stores of the hand-off would come back only after all of them.  (The build
    // switches the compiler's atomic optimizer off: it rewrites a one-lane atomic with a returned value into a wave-wide
    // form that waits for the return on the spot.)  Measured and dropped: taking the ticket a step earlier (after the
    // collision stage of the item's last step: +0.3 % on 20-step launches, -0.2 % on 50-step ones).
    unsigned int t_new = 0;
    if (chunked && lane == 0) t_new = atomicAdd(&st.csched->ticket, 1u);
    {
      // the world's running sums of this launch: lane 1 steps, 2 contacts, 3 solver iterations, 4 overflow steps (integers as
      // bit patterns), 5 shader cycles (float).  Inner items pass them on with the state; the final item adds them to the
      // world's counters — integer adds it does not wait for (uint32: exact up to 4.29e9 — at ~6 contacts per step that
      // is 7e8 steps of one world between two resets)
      const unsigned int own = lane == 1 ? (unsigned int)(step1 - step0) : lane == 2 ? sum_con : lane == 3 ? sum_it : sum_of;
      const float cyc = (float)(__builtin_amdgcn_s_memtime() - t_begin);
      if (lane >= 1 && lane <= 4) carry += own;
      if (lane == 5) carry = __float_as_uint(__uint_as_float(carry) + cyc);
      const bool final = step1 == n_steps;
      if (lane == 6 || lane == 7) add_count(&st.stats_sum[16 * (size_t)w + opaque(lane) - 2], lane == 6 ? sum_dual : sum_kkt);      // (every item adds its own)
      write_outputs(s, m, st, w, lane, time, final, epoch * 32u + (unsigned int)(chunk + 1), carry);
      if (final) {
        if (lane >= 1 && lane <= 4) add_count(&st.stats_sum[16 * (size_t)w + opaque(lane) - 1], carry);
        if (lane == 5) st_state(&st.cost[w], __uint_as_float(carry));     // the world's cycles over the whole launch
      }
      if (st.sched && lane == 0) atomicMax(&st.sched->t_last, (unsigned long long)__builtin_amdgcn_s_memrealtime());
    }
    if (!chunked) break;
    TRACE_SUB(0);
    t_next = (unsigned int)__builtin_amdgcn_readfirstlane((int)t_new);      // scalar across the loop's back edge
    TRACE_SUB(1);
    WSYNC();      // the next item's state loads overwrite the LDS the stores above read
  }
  TRACE_FLUSH();
  if (blockIdx.x == 0 && lane == 0 && st.clock_probe) {      // the clock this launch ran at (nmf_shader_clock)
    atomicAdd(&st.clock_probe[0], __builtin_amdgcn_s_memtime() - probe_c0);
    atomicAdd(&st.clock_probe[1], __builtin_amdgcn_s_memrealtime() - probe_r0);
  }
  STAGE(16);
  STAGE_FLUSH();
}

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
#include "nmf_tree.h"
namespace nmf {

using FlyTopo = Topo<6, 3, 2, 1, 1, 1, 1, 1, 1>;   // LEGS_ONLY skeleton: 49 bodies, 72 dofs
// the full-body skeletons: 20 bodies / 60 dofs of head, antennae, proboscis, abdomen, wings, halteres (tree sweeps) + the
// six legs (unrolled chain sweeps)
using FlyTopoBio = HybridTopo<20, 60, 6, 3, 2, 1, 1, 1, 1, 1, 1>;        // ALL_BIOLOGICAL: 69 bodies, 132 dofs
using FlyTopoAll = HybridTopo<20, 60, 6, 3, 3, 3, 3, 3, 3, 3, 3>;        // ALL_POSSIBLE:   69 bodies, 210 dofs
using FlyTopoActive = Topo<6, 3, 2, 1, 1>;         // LEGS_ACTIVE_ONLY skeleton: 25 bodies, 48 dofs

#if NMF_HAS_TOPO(0)
template __global__ void nmf_step_kernel<FlyTopo, false>(const DevModel*, DevState, ReplayArgs, int);
template __global__ void nmf_step_kernel<FlyTopo, true>(const DevModel*, DevState, ReplayArgs, int);
template __global__ void nmf_step_kernel<Terrain<FlyTopo>, false>(const DevModel*, DevState, ReplayArgs, int);     // terrain worlds (never tethered)
#endif
#if NMF_HAS_TOPO(1)
template __global__ void nmf_step_kernel<FlyTopoActive, false>(const DevModel*, DevState, ReplayArgs, int);
template __global__ void nmf_step_kernel<FlyTopoActive, true>(const DevModel*, DevState, ReplayArgs, int);
template __global__ void nmf_step_kernel<Terrain<FlyTopoActive>, false>(const DevModel*, DevState, ReplayArgs, int);     // terrain worlds (never tethered)
#endif
#if NMF_HAS_TOPO(2)
template __global__ void nmf_step_kernel<TreeTopoSmall, false>(const DevModel*, DevState, ReplayArgs, int);
template __global__ void nmf_step_kernel<TreeTopoSmall, true>(const DevModel*, DevState, ReplayArgs, int);
template __global__ void nmf_step_kernel<Terrain<TreeTopoSmall>, false>(const DevModel*, DevState, ReplayArgs, int);     // terrain worlds (never tethered)
#endif
#if NMF_HAS_TOPO(3)
template __global__ void nmf_step_kernel<TreeTopo, false>(const DevModel*, DevState, ReplayArgs, int);
template __global__ void nmf_step_kernel<TreeTopo, true>(const DevModel*, DevState, ReplayArgs, int);
template __global__ void nmf_step_kernel<Terrain<TreeTopo>, false>(const DevModel*, DevState, ReplayArgs, int);     // terrain worlds (never tethered)
#endif
#if NMF_HAS_TOPO(4)
template __global__ void nmf_step_kernel<FlyTopoBio, false>(const DevModel*, DevState, ReplayArgs, int);
template __global__ void nmf_step_kernel<FlyTopoBio, true>(const DevModel*, DevState, ReplayArgs, int);
template __global__ void nmf_step_kernel<Terrain<FlyTopoBio>, false>(const DevModel*, DevState, ReplayArgs, int);     // terrain worlds (never tethered)
#endif
#if NMF_HAS_TOPO(5)
template __global__ void nmf_step_kernel<FlyTopoAll, false>(const DevModel*, DevState, ReplayArgs, int);
template __global__ void nmf_step_kernel<FlyTopoAll, true>(const DevModel*, DevState, ReplayArgs, int);
template __global__ void nmf_step_kernel<Terrain<FlyTopoAll>, false>(const DevModel*, DevState, ReplayArgs, int);     // terrain worlds (never tethered)
#endif

}  // namespace nmf
