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
//
// This file is the schedule: which stage header comes when, what a launch stages once (stage_launch_constants), the reset
// kernel, the stepping kernel with its chunk scheduler, and the instantiations.  The stages themselves:
#include "nmf_device.h"
#include "nmf_step_lds.h"          // FlyLds and its overlays, layout constants, lane roles
#include "nmf_step_diag.h"         // STAGE / SUB / TRACE macros (diagnostic builds)
#include "nmf_tree_fwd.h"          // what the stage headers call of nmf_tree.h, declared
#include "nmf_step_kinematics.h"   // stage_kinematics, stage_inertia
#include "nmf_step_collision.h"    // terrain, stage_collision
#include "nmf_step_aba.h"          // chain sweeps, aba_solve
#include "nmf_step_contact.h"      // contact rows in registers
#include "nmf_dual.h"              // constraint solve in contact space
#include "nmf_step_noslip.h"       // noslip pass of the primal path
#include "nmf_step_actuation.h"    // control prefetch, general actuators
#include "nmf_step_forward.h"      // physics_forward, physics_integrate
#include "nmf_step_io.h"           // state in / out, tagged granules, pose outputs
#include "nmf_tree.h"              // general-tree / rest-of-body sweeps (last: built from the pieces of nmf_step_aba.h)

namespace nmf {

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
        q[14 + c] = __int_as_float(sym_idx(i, jx));
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
  if constexpr (kEulerFused<TP>) {
    if (lane == 0) {
      const unsigned long long p = (unsigned long long)(st.dual_scratch + (size_t)blockIdx.x * euler_scratch_floats<TP>());
      s.euler_fac[0] = (unsigned int)p; s.euler_fac[1] = (unsigned int)(p >> 32);
    }
  }
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
      // the control row of the current step: the one modulo of the item; the step loop advances it a row at a time and
      // wraps it by a compare (kStepCursor, nmf_step_lds.h; the step loop's own modulos are the old form)
      int row = 0;
      if constexpr (kStepCursor<TP>) {
        if (tab) row = (rp.start + step0) % rp.table_steps;
        pf.value = my_ctrl >= 0 ? tab[(size_t)row * rp.n_act + lane] : 0.f;     // the item's first row travels with the state
      } else pf.value = my_ctrl >= 0 ? tab[(size_t)((rp.start + step0) % rp.table_steps) * rp.n_act + lane] : 0.f;
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
          if constexpr (kStepCursor<TP>) {
            if constexpr (TP::kCtrl > kWave) {     // (more than 64 controls: the 96-control hybrid and the tree kernels)
              const float* src = tab + (size_t)row * rp.n_act;
              for (int a = opaque(lane) + kWave; a < rp.n_act; a += kWave) s.ctrl[rp.act_ids[a]] = src[a];
            }
            row = row + 1 == rp.table_steps ? 0 : row + 1;
            pf.next_row = step + 1 < step1 ? tab + (size_t)row * rp.n_act : nullptr;
          } else {
            const float* src = tab + (size_t)((rp.start + step) % rp.table_steps) * rp.n_act;
            for (int a = opaque(lane) + kWave; a < rp.n_act; a += kWave) s.ctrl[rp.act_ids[a]] = src[a];     // (more than 64 controls: hybrid / tree kernels)
            pf.next_row = step + 1 < step1 ? tab + (size_t)((rp.start + step + 1) % rp.table_steps) * rp.n_act : nullptr;
          }
          WSYNC();
        }
        STAGE(0);
        // an observation ring records this step: its row (wave-uniform address).  (Launches without a ring never reach the
        // modulo; a countdown carried across the loop in its place cost every leg-chain kernel a spilled register: dropped)
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

// One kernel per family of NMF_FAMILIES (nmf_families.h) and world kind: plain, tethered (weld), terrain (never tethered)
#define NMF_INSTANTIATE(k, TP, ...) NMF_IF_TOPO_##k(                                                      \
  template __global__ void nmf_step_kernel<TP, false>(const DevModel*, DevState, ReplayArgs, int);        \
  template __global__ void nmf_step_kernel<TP, true>(const DevModel*, DevState, ReplayArgs, int);         \
  template __global__ void nmf_step_kernel<Terrain<TP>, false>(const DevModel*, DevState, ReplayArgs, int);)
NMF_FAMILIES(NMF_INSTANTIATE)
#undef NMF_INSTANTIATE

}  // namespace nmf
