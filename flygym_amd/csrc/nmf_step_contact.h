// nmf_step_contact.h — constraint rows held in registers: lane = contact (ContactRegs: four pyramid rows each), lanes 48..53 the
// tether weld (WeldRow).  impedance / reference accelerations, the constraint cost, contact_sweep (row forces -> contact
// wrenches in c_w -> J^T f through sweep_project) and contact_project, contact_row_forces.  Reads c_r, c_D, c_mu, c_info and the
// twists in T.
//
// Not self-contained: one of the stage headers that nmf_step.hip includes in stage order to form the stepping kernel's
// translation unit, and it relies on the ones before it.
#pragma once
#include "nmf_device.h"

namespace nmf {

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
