// nmf_step_forward.h — the step itself.  physics_forward runs the stages in order (kinematics, inertia, collision, contact
// parameters, velocities and bias forces, actuation, smooth solve, constraint solve in contact space or by the primal Newton
// loop, sensors) and leaves the constraint forces as contact wrenches in c_w (returns true) or as J^T f in vD; physics_integrate
// is the semi-implicit Euler step on top of them.  This kernel sits at 256 VGPRs: its stage columns move with any change of the
// source.
//
// Not self-contained: one of the stage headers that nmf_step.hip includes in stage order to form the stepping kernel's
// translation unit, and it relies on the ones before it.
#pragma once
#include "nmf_device.h"

namespace nmf {

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
  if constexpr (!kInertiaInKin<TP>) stage_inertia(s, m, lane);      // (leg-chain kernels: inside stage_kinematics)
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
      // Tethered worlds: after a move the gradient is evaluated afresh from the qacc and the row residuals the loop holds, as the
      // oracle does, not carried.  The Euler step solves (M + hB) a = qfrc_smooth + JT f = M qacc − grad with the forces of
      // those residuals, so what is left of their gradient enters the new velocity through M⁻¹, not through H⁻¹, and the weld
      // rows make H = M + JT D J stiffer than M by d / (1 − d) = 49..99 in the root's directions.  The first move from the
      // unconstrained acceleration changes the row forces by that factor times the forces that remain; a gradient carried
      // through it keeps that change's rounding (and its floor, in magv), and the loop ended there with M⁻¹ grad at 1e-5..1e-4 of
      // the step's acceleration where the float32 oracle makes a second move.  Evaluated afresh the gradient is that of the
      // forces the Euler step will read, and the second move takes it down to rounding.
      if constexpr (WELD) {
        if (iter > 0) {
          if (red) {
            if constexpr (TP::kStar) { if constexpr (TP::REST_B > 0) {
              for (int j = lane; j < TP::NV; j += kWave) search[j] = (j >= 6 && j < TP::LD0) ? 0.f : s.qacc[j] - s.qacc_smooth[j];
            } }
            WSYNC();
            mul_M(s, search, m, lane, false, [&](int j, float v) { Gv[j] = v; });
          } else {
            WSYNC();
            mul_M(s, s.qacc, m, lane, false, [&](int j, float v) { Gv[j] = v - s.qfrc_smooth[j]; });
          }
          WSYNC();
          float f0[4] = {0.f, 0.f, 0.f, 0.f};
          if (c.on) contact_row_forces(c, -1.f, f0);
          gn = 0.f; gm = 0.f;
          contact_project<TP, false>(s, c, wr, fr, f0, wr.D * wr.jar, 0.f, m, lane, walls, [&](int j, float proj) {
            const float gv = Gv[j], qs = s.qfrc_smooth[j];
            const float gj = gv + proj;
            const float mag = fabsf(gv + qs) + fabsf(qs) + fabsf(proj);
            rhs[j] = -gj; magv[j] = mag;
            gn += gj * gj; gm += mag * mag;
          });
          gn = wave_sum(gn); gm = wave_sum(gm);
        }
      }
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
    if constexpr (kEulerFused<TP>) aba_solve_stored<TP>(s, V_QFRC_SMOOTH, V_B, m, lane, true);      // (the smooth solve left the factors)
    else aba_solve<TP, WELD, !kDual<TP>>(s, V_QFRC_SMOOTH, V_B, false, h, m, lane, false, true);
  }
  else {
    for (int j = lane; j < s.nv(); j += kWave) s.vA[j] = s.qfrc_smooth[j] + s.vD[j];
    WSYNC();
    if constexpr (kEulerFused<TP>) aba_solve_stored<TP>(s, V_A, V_B, m, lane, false);
    else aba_solve<TP, WELD, !kDual<TP>>(s, V_A, V_B, false, h, m, lane);
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

}  // namespace nmf
