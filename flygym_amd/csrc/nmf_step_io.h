// nmf_step_io.h — how a world's state crosses HBM: agent-scope loads / stores of the state arrays (ld_state / st_state), the
// data-tagged granules that hand a world from one chunk of a launch to the next (st_tagged / ld_tagged), write_outputs (state
// out, pure outputs on the final item) and write_poses (called while the body poses are alive in LDS).
//
// Not self-contained: one of the stage headers that nmf_step.hip includes in stage order to form the stepping kernel's
// translation unit, and it relies on the ones before it.
#pragma once
#include "nmf_device.h"

namespace nmf {

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

}  // namespace nmf
