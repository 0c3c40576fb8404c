// nmf_families.h — the kernel families of the stepping engine: the topology types that state a family's facts, the ONE list
// that numbers the families, and what the host side asks of a family (Family, computed from its type).  To add a family:
// its alias and its row of NMF_FAMILIES below (and a selector NMF_IF_TOPO_k).
//
// Plain C++ without HIP: scripts/micro/classify_check.cpp compiles it on the host.
#pragma once

namespace nmf {

constexpr int kWave = 64;
constexpr int kRestLevels = 6;   // levels below the root the fast passes of the hybrid kernels unroll
constexpr int kMaxCtrl = 48;

// Star-of-chains topology: one free root body + NLEG identical serial chains; DOFS... are the
// hinge counts of the chain's bodies from the root outwards (LEGS_ONLY leg: 3,2,1,1,1,1,1,1).
// Everything about the chain layout is a compile-time constant so that the leg sweeps unroll
// completely and never load structure from memory.
// REST_B / REST_V: bodies / dofs of the "rest" of the fly (head, antennae, proboscis, abdomen, wings, halteres) that sit
// between the root and the legs in the model's order; they are swept by the general-tree code (nmf_tree.h), the legs by
// the unrolled chain code.  Leg-only skeletons have no rest.
template <int REST_B_, int REST_V_, int NLEG_, int... DOFS>
struct HybridTopo {
  static constexpr bool kStar = true;
  static constexpr bool kTerrain = false;   // see Terrain<> below
  // controls a kernel keeps in LDS: 48 for the leg skeletons, 64 for ALL_BIOLOGICAL (which sits exactly on its LDS budget), 96 for
  // ALL_POSSIBLE (the default actuated set on it is 72 leg dofs + 6 adhesion); nmf_batch_create sends models with more
  // actuators to the general-tree kernel, which holds one per dof
  static constexpr int kCtrl = REST_V_ == 0 ? kMaxCtrl : ((DOFS + ...) > 16 ? 96 : 64);
  static constexpr int REST_B = REST_B_, REST_V = REST_V_;
  static constexpr int NLEG = NLEG_;
  static constexpr int NBL = sizeof...(DOFS);
  static constexpr int NDL = (DOFS + ...);
  static constexpr int LB0 = 1 + REST_B_;        // first leg body
  static constexpr int LD0 = 6 + REST_V_;        // first leg dof
  static constexpr int kFact0 = 6, kSlot0 = 1;   // the rest dofs / bodies only (tree sweeps); legs and root keep theirs in registers
  static constexpr int kNFact = REST_V_ > 0 ? REST_V_ : 1, kNSlot = REST_B_ > 0 ? REST_B_ : 1;
  static constexpr int kTblB = 1 + REST_B_, kTblV = 6 + REST_V_;   // tree tables: root + rest bodies, root + rest dofs
  static constexpr int NB = LB0 + NLEG_ * NBL;
  static constexpr int NV = LD0 + NLEG_ * NDL;
  static constexpr int NQ = NV + 1;
  static constexpr int dofs(int l) { constexpr int t[] = {DOFS...}; return t[l]; }
  static constexpr int first_dof(int l) { int a = 0; for (int i = 0; i < l; ++i) a += dofs(i); return a; }
  static constexpr int lbody(int d) { int a = 0; for (int l = 0; l < NBL; ++l) { a += dofs(l); if (d < a) return l; } return NBL - 1; }
  static constexpr bool is_last(int d) { return d == first_dof(lbody(d)) + dofs(lbody(d)) - 1; }
  static constexpr bool is_first(int d) { return d == first_dof(lbody(d)); }
};
template <int NLEG_, int... DOFS>
using Topo = HybridTopo<0, 0, NLEG_, DOFS...>;

// A general kinematic tree (nmf_tree.h): LDS arrays sized for NB_ bodies / NV_ dofs, the actual counts are run-time
// values of the model.  Two sizes are built: 72 x 144 (ALL_BIOLOGICAL: 69 bodies, 132 dofs; 4 flies per CU) and
// 72 x 216 (ALL_POSSIBLE: 210 dofs; 3 flies per CU).
template <int NB_, int NV_>
struct TreeTopoT {
  static constexpr bool kStar = false;
  static constexpr bool kTerrain = false;
  static constexpr int NB = NB_, NV = NV_, NQ = NV_ + 1;
  static constexpr int kCtrl = NV_ + 8;      // every dof actuated + adhesion
  static constexpr int kFact0 = 0, kSlot0 = 1;      // every dof has articulated-body factors, every non-root body a hand-off slot
  static constexpr int kNFact = NV_, kNSlot = NB_;
  static constexpr int kTblB = NB_, kTblV = NV_;
};
// The same skeleton in a world with a terrain (gapped / blocks / mixed: cells with tops and side faces).  A compile-time
// property of the kernel: the collision stage against the cells, contacts with their own frames (a side face's normal is
// horizontal) in every stage that uses the contact frame.  Flat and tethered worlds run the kernels without any of it —
// the same code, registers and LDS as before the terrain's side faces existed.
template <class TP>
struct Terrain : TP {
  static constexpr bool kTerrain = true;
};
using TreeTopo = TreeTopoT<72, 216>;
using TreeTopoSmall = TreeTopoT<72, 144>;
using FlyTopo = Topo<6, 3, 2, 1, 1, 1, 1, 1, 1>;   // LEGS_ONLY skeleton: 49 bodies, 72 dofs
using FlyTopoActive = Topo<6, 3, 2, 1, 1>;         // LEGS_ACTIVE_ONLY skeleton: 25 bodies, 48 dofs
// the full-body skeletons: 20 bodies / 60 dofs of head, antennae, proboscis, abdomen, wings, halteres (tree sweeps) + the
// six legs (unrolled chain sweeps)
using FlyTopoBio = HybridTopo<20, 60, 6, 3, 2, 1, 1, 1, 1, 1, 1>;        // ALL_BIOLOGICAL: 69 bodies, 132 dofs
using FlyTopoAll = HybridTopo<20, 60, 6, 3, 3, 3, 3, 3, 3, 3, 3>;        // ALL_POSSIBLE:   69 bodies, 210 dofs

// The families: X(number, topology type, fallback residency, chunk_div on flat ground).  The number is ABI (nmf_batch_info
// column 0) and the row's index.  with_topo and step_kernel (nmf_capi.hip), the instantiations of nmf_step_kernel
// (nmf_step.hip) and kFamilies below are generated from this list.  The last two columns are measured, not derived:
//  * fallback residency — flies (= single-wave workgroups) a CU holds at once where the runtime does not say (pick_kernel):
//    the LDS-limited figures of the shipped build;
//  * chunk_div, the library's own chunk plan (set_schedule) — flat ground, leg-chain skeleton: a world's cost varies least
//    and a step is cheapest against the hand-over — fewer, longer chunks; terrains and the full-body skeletons keep the
//    halving plan: blocks 34.2 vs 32.4 M, ALL_BIOLOGICAL 30.7 vs 30.2 M
//    (and launches of more than 64 steps: 250-step launches 56.1 M halving, 54.5 M with 1.6)
//    (round 5, one contact-space solve for every walking step: 1.5 / 1.6 / 1.7 / 1.8 / 2.0 = 56.7 / 56.6 / 56.7 / 56.6 / 55.8 M
//    on 20-step launches, 58.7 / 58.9 / 59.2 / 59.0 / 58.9 M on 50-step ones)
#define NMF_FAMILIES(X)                                  \
  X(0, FlyTopo, 8, 1.7)       /* LEGS_ONLY */            \
  X(1, FlyTopoActive, 8, 1.7) /* LEGS_ACTIVE_ONLY */     \
  X(2, TreeTopoSmall, 4, 2.0) /* general tree */         \
  X(3, TreeTopo, 3, 2.0)      /* general tree, large */  \
  X(4, FlyTopoBio, 8, 2.0)    /* ALL_BIOLOGICAL */       \
  X(5, FlyTopoAll, 5, 2.0)    /* ALL_POSSIBLE */

// NMF_TOPO_MASK (development builds only: `scripts/build_variant.sh x -DNMF_TOPO_MASK=1` compiles the LEGS_ONLY kernels alone,
// in a sixth of the time): bit k keeps the kernels of family k of NMF_FAMILIES.  The shipped library has all of them.
// NMF_IF_TOPO_k(code) is `code` where the build has family k and nothing elsewhere: what the list's users wrap kernels in.
#ifndef NMF_TOPO_MASK
#define NMF_TOPO_MASK 0x3f
#endif
#define NMF_HAS_TOPO(k) ((NMF_TOPO_MASK >> (k)) & 1)
#define NMF_KEEP(...) __VA_ARGS__
#define NMF_DROP(...)
#if NMF_HAS_TOPO(0)
#define NMF_IF_TOPO_0 NMF_KEEP
#else
#define NMF_IF_TOPO_0 NMF_DROP
#endif
#if NMF_HAS_TOPO(1)
#define NMF_IF_TOPO_1 NMF_KEEP
#else
#define NMF_IF_TOPO_1 NMF_DROP
#endif
#if NMF_HAS_TOPO(2)
#define NMF_IF_TOPO_2 NMF_KEEP
#else
#define NMF_IF_TOPO_2 NMF_DROP
#endif
#if NMF_HAS_TOPO(3)
#define NMF_IF_TOPO_3 NMF_KEEP
#else
#define NMF_IF_TOPO_3 NMF_DROP
#endif
#if NMF_HAS_TOPO(4)
#define NMF_IF_TOPO_4 NMF_KEEP
#else
#define NMF_IF_TOPO_4 NMF_DROP
#endif
#if NMF_HAS_TOPO(5)
#define NMF_IF_TOPO_5 NMF_KEEP
#else
#define NMF_IF_TOPO_5 NMF_DROP
#endif

// What the host side asks of a family, whether or not the build has its kernels
struct Family {
  int id, per_cu;           // per_cu, chunk_div: the list's measured columns
  double chunk_div;
  bool star;                // a root with identical leg chains (with or without a rest of the body), else a general tree
  int nb, nv, ctrl, n_fact;                        // NB, NV, kCtrl, kNFact
  int rest_b, rest_v, nleg, nbl, ndl, lb0;         // star families
  int dofs[8];                                     // ... hinges of the leg's bodies, root outwards
  constexpr bool legs_only() const { return star && rest_b == 0; }      // leg chains, no rest body
  constexpr bool hybrid() const { return star && rest_b > 0; }          // legs unrolled, rest as a tree: the rest-pack fast path applies
  constexpr bool tree_tables() const { return n_fact > 1; }             // the kernel sweeps tree tables: they are uploaded
};
template <class TP>
constexpr Family describe(int id, int per_cu, double chunk_div) {
  Family f{};
  f.id = id; f.per_cu = per_cu; f.chunk_div = chunk_div;
  f.star = TP::kStar; f.nb = TP::NB; f.nv = TP::NV; f.ctrl = TP::kCtrl; f.n_fact = TP::kNFact;
  if constexpr (TP::kStar) {
    static_assert(TP::NBL <= 8, "Family::dofs");
    f.rest_b = TP::REST_B; f.rest_v = TP::REST_V; f.nleg = TP::NLEG; f.nbl = TP::NBL; f.ndl = TP::NDL; f.lb0 = TP::LB0;
    for (int l = 0; l < TP::NBL; ++l) f.dofs[l] = TP::dofs(l);
  }
  return f;
}
#define NMF_DESCRIBE(k, TP, per_cu, chunk_div) describe<TP>(k, per_cu, chunk_div),
constexpr Family kFamilies[] = {NMF_FAMILIES(NMF_DESCRIBE)};
#undef NMF_DESCRIBE
constexpr bool families_numbered() { int k = 0; for (const Family& f : kFamilies) if (f.id != k++) return false; return true; }
static_assert(families_numbered(), "a family's number is its index in NMF_FAMILIES");
inline const Family& family(int id) { return kFamilies[id]; }

}  // namespace nmf
