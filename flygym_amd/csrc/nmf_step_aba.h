// nmf_step_aba.h — chain sweeps and articulated-body solves in the (leg, component) lane layout: for_dofs / for_bodies,
// sweep_twists (x -> T), sweep_project (W -> S . W), mul_M, the inertia row maps (Ib rows through InertiaRowMap, Isym), the
// contact stiffness rows (KLane, add_contact_K_row), the solves' shared pieces — aba_step_core behind aba_step / aba_step_scaled,
// aba_root_factor, ChainLane (lane set-up), FreeJointAxes, sub_contact_wrenches, aba_forward_sweep — and aba_solve /
// aba_solve_stored, which are written with them.  aba_solve reads a right-hand side and writes a
// solution by vector id (FlyLds::vec), leaves T = twists(x), borrows T..W for the leg -> root hand-off (AbaHandoff) and, for the
// contact-space solve, parks its factors where the dual_* accessors of this file say (c_w + c_m3, vA..vD or the workgroup's
// scratch in HBM).  On the leg-chain kernels the smooth solve's sweep also builds the Euler step's factors, which
// aba_solve_stored then solves on (kEulerFused).
//
// Not self-contained: one of the stage headers that nmf_step.hip includes in stage order to form the stepping kernel's
// translation unit, and it relies on the ones before it.
#pragma once
#include "nmf_device.h"

namespace nmf {

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
    for (int c = 0; c < 6; c++) acc += s.restA[sym_idx(r, c)] * tv[c];
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
// one articulated-body elimination step for hinge/axis `sj` (6 floats, group-uniform) with this lane's row IA, bias component
// pA, own axis component `sown`, diagonal term delta and generalized force tauj: the arithmetic (row products in packed float32)
// and the downdate; aba_step / aba_step_scaled below differ in what they hand back only.  MASKED: `sown` still carries the
// shadow rows' copy of row 5 and is masked here (after U, where aba_step always took the product: the order is in the code).
// MFMA: the downdate on the matrix pipe (grp8_rank1_mfma, nmf_device.h; kAbaRank1Mfma).
template <bool MFMA, bool MASKED>
__device__ __forceinline__ void aba_step_core(float (&IA)[6], float& pA, const float* sj, float sown, float mask, float delta, float tauj,
                                              float& U, float& u, float& invD, float& k) {
  f2 a01 = mk2(IA[0], IA[1]), a23 = mk2(IA[2], IA[3]), a45 = mk2(IA[4], IA[5]);
  f2 acc = a01 * mk2(sj[0], sj[1]);
  acc = __builtin_elementwise_fma(a23, mk2(sj[2], sj[3]), acc);
  acc = __builtin_elementwise_fma(a45, mk2(sj[4], sj[5]), acc);
  U = acc.x + acc.y;
  const float sr = MASKED ? mask * sown : sown;
  const float D = grp8_sum(sr * U) + delta;
  const float sp = grp8_sum(sr * pA);
  invD = __builtin_amdgcn_rcpf(D);
  u = tauj - sp;
  k = U * invD;
  if constexpr (MFMA) grp8_rank1_mfma(IA, -k, U);
  else {
    const f2 nk = mk2(-k, -k);
    a01 = __builtin_elementwise_fma(nk, mk2(grp8_bcast<0>(U), grp8_bcast<1>(U)), a01);
    a23 = __builtin_elementwise_fma(nk, mk2(grp8_bcast<2>(U), grp8_bcast<3>(U)), a23);
    a45 = __builtin_elementwise_fma(nk, mk2(grp8_bcast<4>(U), grp8_bcast<5>(U)), a45);
    IA[0] = a01.x; IA[1] = a01.y; IA[2] = a23.x; IA[3] = a23.y; IA[4] = a45.x; IA[5] = a45.y;
  }
  pA += k * u;
}
// the rest-of-body passes (nmf_tree.h): own component `sown` unmasked; hands back U (shadow rows zero), u and 1 / D
__device__ __forceinline__ void aba_step(float (&IA)[6], float& pA, const float* sj, float sown, float mask, float delta,
                                         float tauj, float& Uout, float& uout, float& invDout) {
  float U, k;
  aba_step_core<false, true>(IA, pA, sj, sown, mask, delta, tauj, U, uout, invDout, k);
  Uout = mask * U;
}
// the leg chains of the star sweeps, whose back-substitution needs (u - U.a) / D only: hands back U / D and u / D (one register
// per dof less to keep, one multiply per dof less in the forward sweep).  SHADOW0: the forward sweep keeps its accelerations
// zero in the shadow rows, so U / D needs no mask either.
template <bool SHADOW0, bool MFMA = false>
__device__ __forceinline__ void aba_step_scaled(float (&IA)[6], float& pA, const float* sj, float sr, float mask, float delta,
                                                float tauj, float& UDout, float& uDout, float& Uraw, float& invDraw) {
  float u, k;
  aba_step_core<MFMA, false>(IA, pA, sj, sr, mask, delta, tauj, Uraw, u, invDraw, k);
  UDout = SHADOW0 ? k : mask * k; uDout = u * invDraw;
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

// Euler's factors (kEulerFused, nmf_step_lds.h): the workgroup's slot — rows of 8 floats, [hinge tip to base][leg], then the
// root's six — with the base address in scalar registers; callers add a lane offset (one vector register) and the step's row
// (in the instruction)
typedef __attribute__((address_space(1))) float* euler_fac_ptr;
template <class TP> __device__ __forceinline__ euler_fac_ptr euler_fac_base(FlyLds<TP>& s) {
  if constexpr (kEulerFused<TP>) {
    const unsigned int lo = (unsigned int)__builtin_amdgcn_readfirstlane((int)s.euler_fac[0]);
    const unsigned int hi = (unsigned int)__builtin_amdgcn_readfirstlane((int)s.euler_fac[1]);
    return (euler_fac_ptr)((unsigned long long)hi << 32 | lo);
  } else return nullptr;
}
// The root's six axes in elimination order: angular z, y, x, then linear z, y, x (both solves; the contact-space solve's root
// factors, nmf_dual.h, are stored in it)
constexpr int dual_root_axis(int i) { return i < 3 ? 2 - i : 8 - i; }
// one root axis of the factor half of the root's elimination (both chains of aba_solve's root block): U is column e of IA (unit
// axes), D its own entry; hands back U, U / D and 1 / D.  MFMA: the downdate on the matrix pipe, D's broadcast on the vector pipe.
template <int e, bool MFMA = false>
__device__ __forceinline__ void aba_root_factor(float (&IA)[6], float& Uout, float& kout, float& invDout) {
  const float U = IA[e];
  Uout = U;
  if constexpr (MFMA) {
    const float invD = __builtin_amdgcn_rcpf(grp8_bcast_dpp<e>(U));
    const float k = U * invD;
    grp8_rank1_mfma(IA, -k, U);
    kout = k; invDout = invD;
    return;
  }
  const float b0 = grp8_bcast<0>(U), b1 = grp8_bcast<1>(U), b2 = grp8_bcast<2>(U), b3 = grp8_bcast<3>(U),
              b4 = grp8_bcast<4>(U), b5 = grp8_bcast<5>(U);
  const float D = e == 0 ? b0 : e == 1 ? b1 : e == 2 ? b2 : e == 3 ? b3 : e == 4 ? b4 : b5;
  const float invD = __builtin_amdgcn_rcpf(D);
  const float k = U * invD;
  { const float bb[6] = {b0, b1, b2, b3, b4, b5}; fma6(IA, -k, bb); }
  kout = k; invDout = invD;
}

// pA -= component rr of the contact wrenches c0 .. c1 - 1 (dual_wrench), as a body force.  ROLLED: the loop as it stands (in the
// chain's backward sweep, where it sits once per body); the root's, once per solve, is left to the optimizer
template <bool ROLLED, class TP>
__device__ __forceinline__ void sub_contact_wrenches(float& pA, FlyLds<TP>& s, int c0, int c1, int rr) {
  if constexpr (ROLLED) {
#pragma clang loop unroll(disable) vectorize(disable)
    for (int c = c0; c < c1; ++c) pA -= dual_wrench(s)[c][rr];
  } else {
    for (int c = c0; c < c1; ++c) pA -= dual_wrench(s)[c][rr];
  }
}


// What a lane of either solve knows about its leg chain.  Shadow rows (r = 6, 7): where S and T have a padding column (S's is
// zeroed at launch) they read their axis component from it and keep the acceleration sweep's value there: zero contributions to
// every group sum without a mask multiply per dof (kShadow0).  Without padding they shadow row 5 and the sums are masked.
// (L is the solve's own lane role, by reference: the column select below is then compiled where the solve is, as it was.)
template <class TP>
struct ChainLane {
  static constexpr bool kShadow0 = row_width_s<TP>() > 6 && row_width_tw<TP>() > 6;
  static constexpr int SW = row_width_s<TP>();
  const LaneRole& L;
  int j0, b0;                 // the leg's first dof / body
  int rS;                     // the lane's column of S and T
  lds_cptr Sleg, Sown;        // the leg's first axis / the lane's own component of it (rows SW apart)
  __device__ __forceinline__ ChainLane(FlyLds<TP>& s, const LaneRole& L_) : L(L_) {
    j0 = TP::LD0 + L.lg * TP::NDL; b0 = TP::LB0 + L.lg * TP::NBL;
    rS = kShadow0 && L.r >= 6 ? 6 : L.rr;
    Sleg = lds_pinned(&s.S[j0][0]); Sown = lds_pinned(&s.S[j0][rS]);
  }
  // the contact ranges of the leg's bodies (cs) and of the root; `any`: some contact term is in the solve (wave-uniform), else empty
  __device__ __forceinline__ void contact_ranges(const FlyLds<TP>& s, bool any, int (&cs)[TP::NBL + 1], int& cs_root0, int& cs_root1) const {
    static_for<TP::NBL + 1>([&](auto I) { constexpr int l = decltype(I)::value; cs[l] = any ? s.body_cstart[b0 + l] : 0; });
    if (any) { cs_root0 = s.body_cstart[0]; cs_root1 = s.body_cstart[1]; }
  }
};

// The free joint's rotation axes.  The root is eliminated in world axes (see aba_solve's root block): generalized forces go in
// as R tau_rot, the rotational accelerations come out as RT alpha.
struct FreeJointAxes {
  float Rm[3][3];                       // Rm[c][k] = component c of the k-th rotation axis of the free joint
  // reads the axes; tw = the wrench of tau[0..5] in world axes (angular, linear)
  template <class TP> __device__ __forceinline__ void load(const FlyLds<TP>& s, const float* tau, float (&tw)[6]) {
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
      for (int c = 0; c < 3; c++) Rm[c][k] = s.S[3 + k][c];
    const float t3 = tau[3], t4 = tau[4], t5 = tau[5];
#pragma unroll
    for (int c = 0; c < 3; c++) { tw[c] = Rm[c][0] * t3 + Rm[c][1] * t4 + Rm[c][2] * t5; tw[3 + c] = tau[c]; }
  }
  // the world-axis accelerations xw (angular, linear) as x[0..5]
  __device__ __forceinline__ void accelerations(const float (&xw)[6], float* x) const {
#pragma unroll
    for (int k = 0; k < 3; k++) {
      x[k] = xw[3 + k];
      x[3 + k] = Rm[0][k] * xw[0] + Rm[1][k] * xw[1] + Rm[2][k] * xw[2];
    }
  }
};

// The forward sweep of both solves: x_j = u_j / D_j - (U_j / D_j) . a,  a += s_j x_j — the root in world axes (linear x, y, z,
// then angular x, y, z: the reverse of dual_root_axis) from Ur / ur, then down the leg from Ureg / ureg; own(d) is the lane's
// own component of the leg's d-th axis.  Writes x, leaves T = twists(x).
template <class TP, class Own>
__device__ __forceinline__ void aba_forward_sweep(FlyLds<TP>& s, float* x, const ChainLane<TP>& C, const FreeJointAxes& R,
                                                  const float (&Ur)[6], const float (&ur)[6], const float (&Ureg)[TP::NDL],
                                                  const float (&ureg)[TP::NDL], Own&& own) {
  const LaneRole& L = C.L;
  float a = 0.f;
  {
    float xw[6];
    static_for<6>([&](auto DD) {
      constexpr int i = decltype(DD)::value;
      constexpr int e = i < 3 ? 3 + i : i - 3;
      const float xe = ur[e] - grp8_sum(Ur[e] * a);
      xw[e] = xe;
      a = (C.kShadow0 ? L.r : L.rr) == e ? a + xe : a;
    });
    R.accelerations(xw, x);
  }
  s.T[0][C.rS] = a;
  static_for<TP::NDL>([&](auto DD) {
    constexpr int d = decltype(DD)::value;
    const float xj = ureg[d] - grp8_sum(Ureg[d] * a);
    x[C.j0 + d] = xj;
    a += xj * own(d);
    if constexpr (TP::is_last(d)) s.T[C.b0 + TP::lbody(d)][C.rS] = a;
  });
  WSYNC();
}

// WITHK_ (leg-chain kernels that have the contact-space solve): the contact stiffness rows are compiled into the solve at all
// — only the primal Newton loop's instantiation has them, so the two solves of an ordinary step (smooth, Euler) run a function
// two thirds the size: the step's hot path has to share a 64 KB instruction cache.  Elsewhere one instantiation serves all.
// RESTRICTION (kEulerFused kernels): the WITHK_ = false instantiation is the SMOOTH SOLVE ONLY — it ignores hdamp and withF
// (hdamp = 0, no wrenches) and overwrites the workgroup's Euler factors; the Euler step's solves are aba_solve_stored.
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
  // kFuse: this instantiation is the smooth solve only (hdamp = 0, no wrenches; Euler's solves are aba_solve_stored) and carries
  // Euler's articulated inertia IAe — the same rows, the diagonal dlt instead of arm — through the same sweep
  constexpr bool kFuse = kEulerFused<TP> && !WITHK_;
  constexpr bool kR1 = kFuse && kAbaRank1Mfma<TP>;      // both chains' downdates on the matrix pipe
  if constexpr (kFuse) { withF = false; hdamp = 0.f; }
  const float* tau = s.vec(tau_id);
  float* x = s.vec(x_id);
  Frame fr{};
  if (withK) fr = ld_frame(s, m);
  const bool walls = TP::kTerrain && withK && __builtin_amdgcn_readfirstlane(s.nwall) != 0;      // terrain side faces in contact this step
  const LaneRole L = lane_role<TP>(lane);
  ChainLane<TP> C(s, L);
  const int j0 = C.j0, b0 = C.b0;
  static_assert(sizeof(AbaHandoff<TP>) <= sizeof(float) * TP::NB * 12, "ABA hand-off does not fit T..W");
  AbaHandoff<TP>& H = *reinterpret_cast<AbaHandoff<TP>*>(&s.T[0][0]);
  // offsets of row rr inside a symmetric 6x6's packed storage (lane constants; the hybrid kernels' hand-off slots)
  int so[6];
#pragma unroll
  for (int c = 0; c < 6; c++) {
    if constexpr (kHasIsym<TP>) so[c] = __float_as_int(s.k_tab[L.rr][14 + c]);
    else { const int i = L.rr < c ? L.rr : c, jx = L.rr < c ? c : L.rr; so[c] = sym_idx(i, jx); }
  }
  InertiaRowMap IM{};                                              // this lane's row of a body's 6x6 inertia, read out of Ib
  if constexpr (!kHasIsym<TP>) IM = inertia_map_unpack(s.k_tab[L.rr]);
  // this lane's row of U_j, S_j; group-uniform u_j, 1/D_j.  Long chains (ALL_POSSIBLE: 24 dofs per leg) re-read S_j in the
  // forward sweep instead of keeping it: 24 registers fewer to spill
  constexpr bool kKeepS = TP::NDL <= 16;
  float Ureg[TP::NDL], ureg[TP::NDL], Sreg[kKeepS ? TP::NDL : 1];        // U / D (this lane's row), u / D, own axis component
  constexpr bool kShadow0 = ChainLane<TP>::kShadow0;
  constexpr int SW = ChainLane<TP>::SW;
  // (rows 0..5 store their U / D, lanes 6, 7 of the group 1 / D: the contact-space factors' idiom below)
  euler_fac_ptr fac = nullptr, fac_root = nullptr;
  if constexpr (kFuse) { fac = euler_fac_base(s) + (L.lg * 8 + (L.r < 6 ? L.r : 6)); fac_root = euler_fac_base(s) + (TP::NLEG * TP::NDL * 8 + (L.r < 6 ? L.r : 6)); }
  KLane KL;                             // contact stiffness rows: per-row constants from the launch's table
  if (withK) {
    const float* q = s.k_tab[L.rr];
#pragma unroll
    for (int i = 0; i < 3; ++i) { KL.dA[i] = q[i]; KL.dB[i] = q[3 + i]; KL.dO[i] = q[6 + i]; }
    KL.ia = __float_as_int(q[9]); KL.ib = __float_as_int(q[10]);
  }
  int cs[TP::NBL + 1], cs_root0 = 0, cs_root1 = 0;                         // contact ranges of the leg's bodies / the root
  C.contact_ranges(s, withK || withF, cs, cs_root0, cs_root1);
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
  float IAe[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};      // (kFuse)
  float pA = 0.f;
  // ---- backward sweep along the leg.  What a hinge reads — its motion subspace, diagonal term and force, and at a body's last
  // hinge the body's inertia row — does not depend on the chain, but LDS takes a wave's operations in order and the sweep also
  // stores (the factors the contact-space solve keeps): a read issued where it is used waits for its own round trip, three
  // times per hinge.  So the reads run ONE HINGE AHEAD of the arithmetic (software pipeline, written out: the stores may alias
  // for all the compiler knows, it will not move a read across them).
  float n_sj[6], n_sown = 0.f, n_delta = 0.f, n_delta_e = 0.f, n_tau = 0.f, n_row[6];
  auto fetch_hinge = [&](auto DN) {
    constexpr int dn = decltype(DN)::value;
#pragma unroll
    for (int i = 0; i < 6; i++) n_sj[i] = C.Sleg[dn * SW + i];
    n_sown = C.Sown[dn * SW];
    n_delta = dof_delta(s, m, j0 + dn, hdamp);
    if constexpr (kFuse) n_delta_e = s.dlt[j0 + dn];
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
    const float sown = n_sown, delta = n_delta, delta_e = n_delta_e, tj = n_tau;
    if constexpr (d > 0) fetch_hinge(std::integral_constant<int, (d > 0 ? d - 1 : 0)>{});
    if constexpr (TP::is_last(d)) {          // entering a new body (going towards the root)
      const int b = b0 + TP::lbody(d);
      if constexpr (kHasIsym<TP>) {
        if constexpr (kDual<TP>) { if (withF) sub_contact_wrenches<true>(pA, s, cs[TP::lbody(d)], cs[TP::lbody(d) + 1], L.rr); }
        if (withK) for (int c = cs[TP::lbody(d)]; c < cs[TP::lbody(d) + 1]; ++c) add_contact_K_row(row, s, c, KL, fr, L.rr, walls);
        add6(IA, row);
        if constexpr (kFuse) add6(IAe, row);
      } else {
        add_inertia_row(IA, s, b, IM);
        if constexpr (kDual<TP>) { if (withF) sub_contact_wrenches<true>(pA, s, cs[TP::lbody(d)], cs[TP::lbody(d) + 1], L.rr); }
        if (withK) for (int c = cs[TP::lbody(d)]; c < cs[TP::lbody(d) + 1]; ++c) add_contact_K_row(IA, s, c, KL, fr, L.rr, walls);
      }
    }
    const float sr = kShadow0 ? sown : L.mask * sown;
    if constexpr (kKeepS) Sreg[d] = sown;        // shadow rows: zero (kShadow0), else row 5's (same T word, same value)
    float Uraw, invDraw;
    aba_step_scaled<kShadow0, kR1>(IA, pA, sj, sr, L.mask, delta, tj, Ureg[d], ureg[d], Uraw, invDraw);
    if constexpr (kFuse) {      // the factor half of the same step on IAe (no right-hand side: that half is dead code here)
      float pe = 0.f, UDe, uDe, Ue, invDe;
      aba_step_scaled<kShadow0, kR1>(IAe, pe, sj, sr, L.mask, delta_e, 0.f, UDe, uDe, Ue, invDe);
      fac[(TP::NDL - 1 - d) * TP::NLEG * 8] = L.r < 6 ? Ue * invDe : invDe;
    }
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
  float legs_row_e[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  static_assert(!kFuse || kLegSumValu, "the fused factor sweep sums the legs on the VALU");
  if constexpr (kLegSumValu) {
    const float gm = L.grp < TP::NLEG ? 1.f : 0.f;
#pragma unroll
    for (int i = 0; i < 6; i++) legs_row[i] = groups_sum(gm * IA[i]);
    if constexpr (kFuse) {
#pragma unroll
      for (int i = 0; i < 6; i++) legs_row_e[i] = groups_sum(gm * IAe[i]);
    }
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
  FreeJointAxes R;
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
    if constexpr (kDual<TP>) { if (withF) sub_contact_wrenches<false>(pA, s, cs_root0, cs_root1, L.rr); }
    if constexpr (kFuse) {      // (the root has no diagonal term: the two chains differ by what the legs hand over)
#pragma unroll
      for (int i = 0; i < 6; i++) IAe[i] = row[i];
      add6(IAe, legs_row_e);
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
    float tw[6];
    R.load(s, tau, tw);
    static_for<6>([&](auto DD) {
      constexpr int i = decltype(DD)::value;
      constexpr int e = dual_root_axis(i);
      float U, k, invD;
      aba_root_factor<e, kR1>(IA, U, k, invD);
      const float sp = grp8_bcast<e>(pA);      // (the right-hand-side half goes round the factor step)
      const float u = tw[e] - sp;
      pA += k * u;
      Ur[e] = kShadow0 ? k : L.mask * k; ur[e] = u * invD;
      if constexpr (kFuse) {
        float Ue, ke, invDe;
        aba_root_factor<e, kR1>(IAe, Ue, ke, invDe);
        fac_root[i * 8] = L.r < 6 ? ke : invDe;
      }
      if constexpr (kDual<TP>) {
        if (store) {
          const float rs = __builtin_sqrtf(invD);
          dual_root(s)[i][L.r < 6 ? L.r : 6] = L.r < 6 ? U * rs : rs;
        }
      }
    });
  }
  aba_forward_sweep(s, x, C, R, Ur, ur, Ureg, ureg, [&](int d) { if constexpr (kKeepS) return Sreg[d]; else return C.Sown[d * SW]; });
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

// The Euler step's solve of (M + h B) x = tau [+ the contact wrenches in c_w as body forces] on the factors the smooth solve of
// the same step left in the workgroup's scratch (kEulerFused): the right-hand-side half of aba_solve's backward sweep — bias
// wrench, s . pA, u, u / D; no inertia, no LDS round trip on the chain — the root's six steps likewise, and aba_solve's forward
// sweep.  Leaves T = twists(x).  A function of its own, not a run-time branch of aba_solve: the step's hot path shares a 64 KB
// instruction cache.
template <class TP>
__device__ __noinline__ void aba_solve_stored(FlyLds<TP>& s, int tau_id, int x_id, const GModel& m, int lane, bool withF) {
  static_assert(kEulerFused<TP> && TP::NLEG <= 8 && TP::NDL <= 16, "leg-chain kernels");
  withF = __builtin_amdgcn_readfirstlane((int)withF) != 0;
  SUB_T0();
  SUB(18);
  // the factors first: their round trip to L2 runs under the right-hand side's reads (the compiler orders the 34 loads as it
  // likes and waits for all of them once, before the first hinge)
  const LaneRole L = lane_role<TP>(lane);
  ChainLane<TP> C(s, L);
  constexpr int NE = TP::NDL + 6;
  float Fk[NE], Fd[NE];      // U / D of this lane's row, 1 / D
  {
    const euler_fac_ptr fk = euler_fac_base(s) + (L.lg * 8 + L.rr), fd = euler_fac_base(s) + (L.lg * 8 + 6);
    const euler_fac_ptr rk = euler_fac_base(s) + (TP::NLEG * TP::NDL * 8 + L.rr), rd = euler_fac_base(s) + (TP::NLEG * TP::NDL * 8 + 6);
#pragma unroll
    for (int e = 0; e < TP::NDL; ++e) { Fk[e] = fk[e * TP::NLEG * 8]; Fd[e] = fd[e * TP::NLEG * 8]; }
#pragma unroll
    for (int i = 0; i < 6; ++i) { Fk[TP::NDL + i] = rk[i * 8]; Fd[TP::NDL + i] = rd[i * 8]; }
  }
  const float* tau = s.vec(tau_id);
  float* x = s.vec(x_id);
  constexpr bool kShadow0 = ChainLane<TP>::kShadow0;
  int cs[TP::NBL + 1], cs_root0 = 0, cs_root1 = 0;                         // contact ranges of the leg's bodies / the root
  C.contact_ranges(s, withF, cs, cs_root0, cs_root1);
  float Ureg[TP::NDL], ureg[TP::NDL], sown[TP::NDL], tj[TP::NDL];      // U / D (this lane's row), u / D, own axis component, force
#pragma unroll
  for (int d = 0; d < TP::NDL; ++d) { sown[d] = C.Sown[d * C.SW]; tj[d] = tau[C.j0 + d]; }
  float pA = 0.f;
  static_for<TP::NDL>([&](auto DD) {
    constexpr int d = TP::NDL - 1 - decltype(DD)::value;
    if constexpr (TP::is_last(d)) {          // entering a new body (going towards the root)
      if (withF) sub_contact_wrenches<true>(pA, s, cs[TP::lbody(d)], cs[TP::lbody(d) + 1], L.rr);
    }
    const float sr = kShadow0 ? sown[d] : L.mask * sown[d];
    const float k = Fk[TP::NDL - 1 - d], invD = Fd[TP::NDL - 1 - d];
    const float sp = grp8_sum(sr * pA);
    const float u = tj[d] - sp;
    pA += k * u;
    Ureg[d] = kShadow0 ? k : L.mask * k; ureg[d] = u * invD;
  });
  const float gm = L.grp < TP::NLEG ? 1.f : 0.f;
  const float legs_pA = groups_sum(gm * pA);
  // ---- root (see aba_solve): world axes, generalized forces in as R tau_rot
  float Ur[6], ur[6];
  FreeJointAxes R;
  {
    pA = 0.f;
    if (withF) sub_contact_wrenches<false>(pA, s, cs_root0, cs_root1, L.rr);
    pA += legs_pA;
    float tw[6];
    R.load(s, tau, tw);
    static_for<6>([&](auto DD) {
      constexpr int i = decltype(DD)::value;
      constexpr int e = dual_root_axis(i);
      const float k = Fk[TP::NDL + i], invD = Fd[TP::NDL + i];
      const float sp = grp8_bcast<e>(pA);
      const float u = tw[e] - sp;
      pA += k * u;
      Ur[e] = kShadow0 ? k : L.mask * k; ur[e] = u * invD;
    });
  }
  aba_forward_sweep(s, x, C, R, Ur, ur, Ureg, ureg, [&](int d) { return sown[d]; });
  SUB(19);      // (the stage profile's "(all ABA) legs + root" row covers this solve as it covers aba_solve)
}

}  // namespace nmf
