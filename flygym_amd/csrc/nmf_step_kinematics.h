// nmf_step_kinematics.h — kinematics and inertia stages.  stage_kinematics reads qpos and leaves the body poses (xmat / xpos:
// overlaid on the solver vectors and the contact wrenches, alive until the end of the collision stage) and the motion subspaces
// S; its scratch is qacc_smooth..vD (joint quaternions), T..W (relative transforms) and Ib (body-frame axes).  stage_inertia
// then rebuilds Ib (and Isym) about the root origin from the poses — in the leg-chain kernels stage_kinematics does so itself,
// last, from constants it requested at its entry (kInertiaInKin, nmf_step_lds.h).
//
// Not self-contained: one of the stage headers that nmf_step.hip includes in stage order to form the stepping kernel's
// translation unit, and it relies on the ones before it.
#pragma once
#include "nmf_device.h"

namespace nmf {

// ------------------------------------------------------------------ inertia of one body
// A body's inertial constants of the model, as stage_kinematics holds them from its entry on (kInertiaInKin): the body-frame
// inertia (xx, yy, zz, xy, xz, yz), the centre of mass and the mass
struct BodyInertial { float q[6], ipos[3], mass; };
__device__ __forceinline__ BodyInertial ld_inertial(const GModel& m, int b) {
  BodyInertial k;
#pragma unroll
  for (int i = 0; i < 6; ++i) k.q[i] = m.body_inertia[6 * b + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) k.ipos[i] = m.body_ipos[3 * b + i];
  k.mass = m.body_mass[b];
  return k;
}
// Ib (and Isym) of body b about the root origin from its pose and its constants in registers: stage_inertia's expressions
template <class TP>
__device__ __forceinline__ void inertia_of_body(FlyLds<TP>& s, int b, const float* q, const float* ipos, const float* mass) {
  {
    const float* R = s.xmat()[b];
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
    V3 c = mat_vec(R, ld3(ipos)) + (ld3(s.xpos()[b]) - ld3(s.xpos()[0]));
    float ms = *mass, cc = dot(c, c);
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
}

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
  // kInertiaInKin: lane b's inertial constants are requested here and used behind the motion subspaces, a stage's length later
  // (requested behind the caller's return instead, the call's drained memory counter put their round trip in front of the
  // inertia stage's first line)
  BodyInertial inertial;
  if constexpr (kInertiaInKin<TP>) {
    static_assert(!kInertiaInKin<TP> || TP::NB <= kWave, "one body per lane");
    if (lane < s.nb()) inertial = ld_inertial(m, lane);
  }
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
  if constexpr (kInertiaInKin<TP>) {     // the pass above read the body-frame axes that lie in Ib: only now is it rebuilt
    if (lane < s.nb()) inertia_of_body(s, lane, inertial.q, inertial.ipos, &inertial.mass);
    WSYNC();
  }
}

// The inertia stage of the kernels whose stage_kinematics does not build Ib itself (kInertiaInKin).  The expressions are those of
// inertia_of_body; they stay spelled out here so that these kernels (256 VGPRs, a spill apart) compile to what they were.
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

}  // namespace nmf
