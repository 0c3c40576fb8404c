// nmf_step_lds.h — what a fly keeps in LDS while it steps, and the vocabulary every stage shares: the stage boundary (WSYNC),
// the SolveReport bits, FlyLds / TreeLds with all their overlays (body poses on the
// solver vectors and the contact wrenches, AbaHandoff and the contact-space solve's Gram matrix on Ib..W, DualFactors on c_w +
// c_m3), the kDual* layout constants, the model's hot part (HotModel), the contact info word, contact frames and the (leg,
// component) lane roles.
//
// Not self-contained: one of the stage headers that nmf_step.hip includes in stage order to form the stepping kernel's
// translation unit, and it relies on the ones before it.
#pragma once
#include "nmf_device.h"

namespace nmf {

// Stage boundaries.  One wave per workgroup, and the LDS unit takes a wave's operations in order: a read that follows
// another lane's write in program order sees it, so a boundary only has to order the accesses for the COMPILER — a
// wavefront-scope fence.  __syncthreads() (the round-1/2 behaviour) additionally parks the wave on `s_waitcnt lgkmcnt(0)`
// until its LDS writes have drained: ~60 times per step, 1.2 % of the launch.
#define WSYNC() do { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)
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
// Leg-chain kernels: the smooth solve's backward sweep carries the Euler step's articulated inertia (diagonal dlt instead of arm)
// beside its own and parks that chain's factors in the workgroup's scratch in HBM (DevState::dual_scratch; these kernels have
// no other use for it): per leg hinge (tip to base) and leg a row of 8 floats — U / D of the six rows, 1 / D, pad —, then one
// such row per root axis (every group eliminates the root redundantly: one copy).  Euler's solve (aba_solve_stored,
// nmf_step_aba.h) is the right-hand-side half of a sweep on them.  Written and read by the same wave within one step, but not
// by the same lanes: 1 / D, stored by lanes 6 and 7 of a group, is read by all eight; a shadow lane reads its twin's word, which
// holds bit for bit what it would have computed; the root's rows, stored by all eight groups (the same values), are read by
// all.  No fence: a wave's vector memory operations reach its CU's L1 in program order, a store and a later load of one wave to
// the same address are served in that order, and non-inlined calls lie between the two (each begins with s_waitcnt vmcnt(0)) —
// what the contact-space factors of kDualGlob rely on as well.  The slot is as small as that (2.3 KB for
// LEGS_ONLY): with a pair per lane and step (8.7 KB) the resident workgroups' slots and their private scratch overflowed an
// XCD's L2 and two thirds of the stores went out to memory (DESIGN_APPENDIX.md section K).
// -DNMF_EULER_REFACTOR: Euler's solve factorises for itself as before, no scratch.
template <class TP> constexpr bool euler_fused() {
#ifdef NMF_EULER_REFACTOR
  return false;
#else
  return has_cm3<TP>();
#endif
}
template <class TP> inline constexpr bool kEulerFused = euler_fused<TP>();
// The fixed cost of a step around its stages (DESIGN_APPENDIX.md section N): the step loop of nmf_step_kernel carries the
// control table's row from step to step and wraps it by a compare instead of taking two run-time modulos per step, and the
// loop for controls 64 and up exists only in kernels that can hold as many.  The hybrid terrain kernels keep the old loop: the
// cursor cost the ALL_BIOLOGICAL one a spilled register.  And in the leg-chain kernels of flat and tethered worlds
// stage_kinematics requests the bodies' inertial constants at its entry and builds Ib / Isym itself, last (kInertiaInKin): the
// model's round trip runs under the stage instead of behind the call's return, in front of the inertia stage's first line.
// (Their terrain kernels keep the inertia stage: with the move the blocks bench lost 0.4 %.)
// -DNMF_STEP_FIXED_OLD: the old loop and the inertia stage everywhere — the machine code from before the change.
template <class TP> constexpr bool step_cursor() {
#ifdef NMF_STEP_FIXED_OLD
  return false;
#else
  if constexpr (TP::kStar) return !(TP::REST_B > 0 && TP::kTerrain); else return true;
#endif
}
template <class TP> constexpr bool inertia_in_kinematics() {
#ifdef NMF_STEP_FIXED_OLD
  return false;
#else
  return has_cm3<TP>() && !TP::kTerrain;
#endif
}
template <class TP> inline constexpr bool kStepCursor = step_cursor<TP>();
template <class TP> inline constexpr bool kInertiaInKin = inertia_in_kinematics<TP>();
// Leg-chain kernels: the rank-1 downdates of the fused smooth solve's two chains (legs and root) run on the matrix pipe
// (grp8_rank1_mfma, nmf_device.h) instead of six group broadcasts through the LDS crossbar and three v_pk_fma_f32 each — the
// same multiply-adds, the same bits.  -DNMF_ABA_RANK1_VALU: the broadcasts and packed multiply-adds everywhere, as before.
template <class TP> constexpr bool aba_rank1_mfma() {
#ifdef NMF_ABA_RANK1_VALU
  return false;
#else
  return euler_fused<TP>();
#endif
}
template <class TP> inline constexpr bool kAbaRank1Mfma = aba_rank1_mfma<TP>();
template <class TP> constexpr int euler_scratch_floats() { if constexpr (has_cm3<TP>()) return 8 * (TP::NLEG * TP::NDL + 6); else return 0; }      // (the leg-chain kernels, whatever the build's switch)
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
  // kEulerFused: address of this workgroup's scratch for Euler's factors in HBM, low and high word (set once per launch;
  // euler_fac_base).  Here because Ib's alignment leaves eight bytes free behind Isym on both leg-chain skeletons: the kernels'
  // LDS stays what it was.  Words, not a pointer: an empty array of pointers would still align what follows to eight bytes and
  // move Ib in the hybrid and tree kernels, which do not have the member's contents.
  unsigned int euler_fac[kEulerFused<TP> ? 2 : 0];
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

}  // namespace nmf
