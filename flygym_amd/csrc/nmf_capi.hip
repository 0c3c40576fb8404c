// nmf_capi.hip — host side of libnmf_hip.so: the C ABI declared in include/nmf.h.
//
// Owns device memory for the model constants and the per-world state, launches the fused step
// kernel (nmf_step.hip) and the gather/scatter kernels (nmf_batch_ops.hip).  No torch types, no host sync on the
// stepping path.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

// NMF_DEVMEM_CHECK: scripts/micro/devmem_check.cpp compiles this file up to DevMem alone, over host stand-ins for its HIP calls
#ifndef NMF_DEVMEM_CHECK
#include <hip/hip_runtime.h>

#include "nmf.h"
#include "nmf_batch_ops.hip"
#include "nmf_step.hip"
#include "nmf_sensors.hip"
// `#pragma clang fp reassociate(off)` at file scope holds from the first file that sets it to the end of the translation unit:
// nmf_scene.h (through nmf_eyes.hip) sets it, so nmf_camera.hip, nmf_replay.hip, nmf_cpg.hip, nmf_plume.hip, nmf_taxis.hip, nmf_odometry.hip, nmf_motion.hip, nmf_navigator.hip, nmf_stabilizer.hip, nmf_rules.hip, nmf_visnet.hip, nmf_task.hip and the host code
// below are all compiled under it, and the files above are not.  Which files it covers decides their kernels' arithmetic: keep the
// order (nmf_taxis.hip, nmf_odometry.hip, nmf_motion.hip, nmf_navigator.hip, nmf_stabilizer.hip, nmf_rules.hip, nmf_visnet.hip and nmf_task.hip add pragmas inside their functions only: nothing of them reaches past the file).
#include "nmf_eyes.hip"
#include "nmf_camera.hip"
#include "nmf_replay.hip"
#include "nmf_cpg.hip"
#include "nmf_plume.hip"
#include "nmf_taxis.hip"
#include "nmf_odometry.hip"
#include "nmf_motion.hip"
#include "nmf_navigator.hip"
#include "nmf_stabilizer.hip"
#include "nmf_rules.hip"
#include "nmf_visnet.hip"
#include "nmf_task.hip"
#include "nmf_skeleton.h"      // nmf_model, the blob parser, classify_skeleton
#endif

namespace {

thread_local std::string g_err;
int fail(const std::string& msg) { g_err = msg; return -1; }

#define HIP_OK(expr)                                                                        \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess) return fail(std::string(#expr) + ": " + hipGetErrorString(e_));   \
  } while (0)

// Makes the batch's device current for the calls below and puts the caller's back on every return path: torch (and any
// other HIP user of the thread) reads its current device through hipGetDevice, so a library call must not change it.
struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  hipError_t err = hipSuccess;
  explicit DeviceGuard(int device) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != device) { err = hipSetDevice(device); switched = err == hipSuccess; }
  }
  ~DeviceGuard() { if (switched && prev >= 0) (void)hipSetDevice(prev); }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define DEVICE_GUARD(b)                                                                       \
  DeviceGuard guard_((b)->mem.device);                                                        \
  if (guard_.err != hipSuccess) return fail(std::string("hipSetDevice: ") + hipGetErrorString(guard_.err))

// The device memory of one handle (batch, eye plan, camera plan, CPG, plume, odometry, motion, navigator, stabilizer, rules, visual network, task): every allocation is 16-byte granular, recorded, and freed
// with the handle.  The first failure sets the error text, named after the entry point `who`, and sticks: later calls return
// null without touching the device, so that a caller tests `ok` once after its last allocation.
struct DevMem {
  int device = 0;
  const char* who = "";
  bool ok = true;
  std::vector<void*> ptrs;

  void* alloc(size_t bytes) { return upload(nullptr, bytes); }       // zero-filled
  void* upload(const void* src, size_t bytes) {                      // a copy of host memory (zeros where src is null)
    if (!ok) return nullptr;
    const size_t size = (std::max(bytes, (size_t)1) + 15) & ~(size_t)15;
    void* p = nullptr;
    if (hipMalloc(&p, size) != hipSuccess) { ok = false; fail(std::string(who) + ": out of device memory"); return nullptr; }
    ptrs.push_back(p);
    if ((src && bytes ? hipMemcpy(p, src, bytes, hipMemcpyHostToDevice) : hipMemset(p, 0, size)) != hipSuccess) {
      ok = false; fail(std::string(who) + ": the upload to the device failed"); return nullptr;
    }
    return p;
  }
  // Frees what was allocated since mark() and clears a failure since then: the handle is as it was at the mark
  size_t mark() const { return ptrs.size(); }
  void rollback(size_t mark) {
    DeviceGuard guard(device);
    for (size_t k = mark; k < ptrs.size(); ++k) (void)hipFree(ptrs[k]);      // (hipFree waits for the kernels that read them)
    ptrs.resize(mark);
    ok = true;
  }
  void release() { rollback(0); }
};

}  // namespace

#ifndef NMF_DEVMEM_CHECK      // (to the end of the file)
namespace {

// The body of a *_create entry point: `fill` builds the fresh handle `h` with its device current.  If it fails the handle is
// destroyed, the error text stays, and the caller gets null.
template <class H, class Fill>
H* build_or_destroy(int device, const char* who, H* h, void (*destroy)(H*), Fill&& fill) {
  h->mem.device = device; h->mem.who = who;
  DeviceGuard guard(device);
  if (guard.err != hipSuccess) fail(std::string("hipSetDevice: ") + hipGetErrorString(guard.err));
  else if (fill(h) == 0) return h;
  const std::string keep = g_err;
  destroy(h);
  g_err = keep;
  return nullptr;
}

}  // namespace

// Visit plan of the eye renderer (nmf_eye_plan_create): everything the kernel reads that depends on the id map, the lens and the
// ommatidia types — with its OWN device copies of the id map, the retina run plan, the pale flags and the normalisation, so that
// a render call is pure stream-ordered work whatever the caller does with its buffers afterwards.
struct nmf_eye_plan {
  int h = 0, w = 0, n_omm = 0;
  float fov = 0.f;
  int n_groups[3] = {0, 0, 0};                 // [0] chunks that feed an ommatidium, [1] all chunks (frames), [2] sampled mode: pixels
  int* visit[3] = {nullptr, nullptr, nullptr};
  float* cones[3] = {nullptr, nullptr, nullptr};
  float* chunk_cones[3] = {nullptr, nullptr, nullptr};
  int* slot_omm = nullptr;
  int16_t* id_map = nullptr; void* rplan = nullptr; uint8_t* pale = nullptr; float* inv_norm = nullptr;      // the plan's copies
  DevMem mem;
  // cache key of nmf_eye_render's implicit plans: the caller's buffer addresses
  const void* key[4] = {nullptr, nullptr, nullptr, nullptr};
};

struct nmf_batch {
  const nmf_model* model = nullptr;
  int n_worlds = 0, topo = 0;
  nmf::DevModel dm{};
  nmf::DevModel* dm_dev = nullptr;
  nmf::DevState st{};
  DevMem mem;
  float* fields[NMF_FIELD_COUNT] = {};
  int widths[NMF_FIELD_COUNT] = {};
  int64_t steps = 0;
  int* order_buf = nullptr;      // block -> world order of the next stepping launch (see nmf_order_kernel)
  nmf::SchedState* sched_buf = nullptr;
  int resident_waves = 0;        // step-kernel waves the device holds at once
  nmf::ChunkSched* csched_buf = nullptr;   // chunked launches (see nmf_step_kernel): ticket / completion / epoch counters
  unsigned long long* handoff_buf = nullptr;   // chunk hand-off granules (nmf_step_kernel); allocated with the batch
  // eye renderer: the visit plan of the last id map it was called with ([0] chunks that touch an ommatidium, [1] all chunks)
  // nmf_eye_render (the entry without an explicit plan handle) keeps the plans it has built: a few, least recently used first out
  std::vector<nmf_eye_plan*> eye_plans;
  int handoff_stride = 0;
  unsigned long long* clock_probe_buf = nullptr;
  const void* step_fn = nullptr; // the stepping kernel this batch launches (nmf_batch_info)
  int per_cu = 0;                // workgroups of it a CU holds
  unsigned lds_pad = 0;          // idle dynamic LDS per workgroup that holds the residency at options.flies_per_cu (0: none)
  bool chunking = true;          // options.sched = 1 keeps whole-launch work items
  // diagnostics: NMF_SCHED = chunks (default) | plain (= NMF_NO_CHUNKS=1); NMF_ORDER = auto (default) | costliest | inorder |
  // none (no order kernel, worlds in index order) | policy (rounds 1-2: in order or costliest first, whichever measured
  // faster, the other re-tried every 32nd launch).  auto = costliest first for launches of up to 64 steps — the cost of the
  // previous launch predicts this one's (20-step CPG launches 43.1 vs 42.5 M env-steps/s, replay 45.9 vs 45.0 M; 50-step
  // 44.7 vs 44.5 M) — and the measured policy for longer ones, whose costs are a third of a gait cycle stale (250-step
  // launches: 43.7 M costliest first, 45.6 M measured policy)
  int order_every = 1, order_age = 0;      // costliest-first order: recomputed every order_every-th launch (NMF_ORDER_EVERY)
  bool order_valid = false;
  int order_policy = 3;          // 3 auto (default), 1 costliest first, 0 in order, 2 none, -1 the measured policy of rounds 1-2
  int max_chunks = 8, min_chunk_steps = 1;   // NMF_MAX_CHUNKS (<= 16) / NMF_MIN_CHUNK_STEPS / NMF_CHUNK_DIV: tuning experiments
  bool chunk_div_short = false;  // chunk_div applies to launches of up to 64 steps only (longer ones halve)
  double chunk_div = 2.0;        // halving chunks; 1.6 (20 = 13 + 5 + 2, 50 = 32 + 12 + 4 + 2) for the leg-chain kernels on flat ground, see launch()
};

extern "C" const char* nmf_last_error(void) { return g_err.c_str(); }

extern "C" nmf_model* nmf_model_create(const void* blob, size_t nbytes) {
  g_err.clear();
  std::string err;
  nmf_model* m = parse_model(blob, nbytes, err);
  if (!m) fail(err);
  return m;
}

extern "C" void nmf_model_destroy(nmf_model* model) { delete model; }

// Most contacts the model's contact set can make in one step: a capsule touches with its two end spheres (and, over a
// terrain with side faces, each of them with one face as well), a hull with up to sem_max_hull_contacts vertices (plus
// one face).  The engine keeps nmf::kMaxCon of them.
extern "C" int nmf_model_contact_bound(const nmf_model* m) {
  if (!m) return fail("nmf_model_contact_bound: null model");
  const HostArray* gt = m->find("geom_type"); const HostArray* so = m->find("sem_options"); const HostArray* tt = m->find("terrain_type");
  if (!gt || !gt->is_int) return fail("nmf_model_contact_bound: model without geom_type");
  const int per_hull = so && so->is_int && so->i.size() > 3 && so->i[3] >= 1 && so->i[3] <= 4 ? so->i[3] : 4;
  const bool faces = tt && tt->is_int && !tt->i.empty() && tt->i[0] != 0 && so && so->i.size() > 4 && so->i[4] != 0;
  int bound = 0;
  for (int t : gt->i) bound += t == nmf::GEOM_CAPSULE ? (faces ? 4 : 2) : per_hull + (faces ? 1 : 0);
  return bound;
}

extern "C" int nmf_batch_set_contact_capacity(nmf_batch* b, int max_contacts) {
  if (!b) return fail("nmf_batch_set_contact_capacity: null batch");
  if (max_contacts < 1) return fail("nmf_batch_set_contact_capacity: max_contacts must be at least 1");
  const int cap = max_contacts > nmf::kMaxCon ? nmf::kMaxCon : max_contacts;
  DEVICE_GUARD(b);      // the caller's current device stays what it was
  b->dm.max_contacts = cap;
  HIP_OK(hipMemcpy(reinterpret_cast<char*>(b->dm_dev) + offsetof(nmf::DevModel, max_contacts), &cap, sizeof(int), hipMemcpyHostToDevice));
  return cap;
}

extern "C" int nmf_model_dims(const nmf_model* m, int32_t out[10]) {
  if (!m) return fail("nmf_model_dims: null model");
  out[0] = m->nq; out[1] = m->nv; out[2] = m->nu; out[3] = m->nb; out[4] = m->nseg; out[5] = m->ng;
  out[6] = m->nsite; out[7] = nmf::kMaxCon; out[8] = 96; out[9] = m->star[0];
  return 0;
}

namespace {

// The batch's copy of a host array.  `slot`: address of a DevModel pointer member (the device pass of this file sees those typed
// as global memory, NMF_G).  A failure is the batch's to test (b->mem.ok).
template <class T>
void upload(nmf_batch* b, const std::vector<T>& host, void* slot) {
  const void* p = b->mem.upload(host.data(), sizeof(T) * host.size());
  memcpy(slot, &p, sizeof(p));
}
int upload_f(nmf_batch* b, const char* name, void* slot) {
  const HostArray* a = b->model->find(name);
  if (!a || a->is_int) return fail(std::string("model lacks float entry ") + name);
  upload(b, a->f, slot);
  return 0;
}
int upload_i(nmf_batch* b, const char* name, void* slot) {
  const HostArray* a = b->model->find(name);
  if (!a || !a->is_int) return fail(std::string("model lacks int entry ") + name);
  upload(b, a->i, slot);
  return 0;
}

// A zeroed device buffer of `count` T that lives as long as the batch
template <class T>
void alloc_dev(nmf_batch* b, size_t count, T** out) { *out = (T*)b->mem.alloc(sizeof(T) * count); }

void alloc_field(nmf_batch* b, int field, int width, float** out) {
  alloc_dev(b, (size_t)b->n_worlds * (size_t)(width > 0 ? width : 1), out);
  b->fields[field] = *out;
  b->widths[field] = width;
}

template <class T> struct TopoTag { using type = T; };

// The kernel family of a batch (nmf_batch::topo) as its topology type: calls f(TopoTag<TP>{}), false for a family this build
// left out (NMF_TOPO_MASK).  Generated from the family list, NMF_FAMILIES (nmf_families.h).
template <class F>
bool with_topo(int topo, F&& f) {
  switch (topo) {
#define NMF_CASE(k, TP, ...) NMF_IF_TOPO_##k(case k: f(TopoTag<nmf::TP>{}); return true;)
    NMF_FAMILIES(NMF_CASE)
#undef NMF_CASE
    default: return false;
  }
}

// The stepping kernel of a family for a tethered (weld), terrain or plain world; nullptr if the build has no such family
const void* step_kernel(int topo, bool weld, bool terrain) {
  const void* fn = nullptr;
  with_topo(topo, [&](auto tag) {
    using TP = typename decltype(tag)::type;
    fn = weld ? reinterpret_cast<const void*>(&nmf::nmf_step_kernel<TP, true>)
              : terrain ? reinterpret_cast<const void*>(&nmf::nmf_step_kernel<nmf::Terrain<TP>, false>)
                        : reinterpret_cast<const void*>(&nmf::nmf_step_kernel<TP, false>);
  });
  return fn;
}

int launch_reset(nmf_batch* b, const uint8_t* mask_dev, hipStream_t stream) {
  DEVICE_GUARD(b);
  with_topo(b->topo, [&](auto tag) {
    hipLaunchKernelGGL((nmf::nmf_reset_kernel<typename decltype(tag)::type>), dim3((unsigned)b->n_worlds), dim3(nmf::kWave), 0, stream,
                       b->dm_dev, b->st, mask_dev);
  });
  HIP_OK(hipGetLastError());
  return 0;
}

struct RingArgs { float* ring = nullptr; int stride = 0, every = 0, nj = 0, nact = 0; };

int launch(nmf_batch* b, const nmf::ReplayArgs& rp, int n_steps, hipStream_t stream, const RingArgs& ring = RingArgs()) {
  DEVICE_GUARD(b);      // the caller's current device need not be the batch's, and stays what it was
  b->st.ring = ring.ring; b->st.ring_stride = ring.stride; b->st.obs_every = ring.ring ? ring.every : 0; b->st.ring_nj = ring.nj; b->st.ring_nact = ring.nact;
  // More worlds than resident waves and a launch long enough to cut: chunks whose lengths shrink towards the end of the
  // launch ("guided" sizes: each takes 1 / chunk_div of what is left, at least min_chunk_steps, at most max_chunks chunks)
  // — long items while there is plenty of other work, short ones where they bound the tail.  Measured on 4096 worlds,
  // round 2: whole-launch items 32.0 / 31.9 M env-steps/s (20- / 50-step launches), 7 equal chunks 36.3 / 38.3 M, halving
  // chunks (chunk_div 2: 10 + 5 + 3 + 1 + 1 steps) 42.4 / 44.4 M; a last chunk of one step (min_chunk_steps 1) is worth
  // +1.2 % on 50-step launches.  Round 4 (a step a quarter cheaper, the hand-over the same): fewer, longer chunks — chunk_div
  // 1.4 / 1.5 / 1.6 / 1.7 / 1.8 / 2.0: 51.4 / 53.4 / 53.6 / 53.4 / 53.3 / 52.5 M on 20-step launches, 53.4 / 54.5 / 55.3 / 55.5 / 55.1 / 55.2 M on 50-step ones.
  const bool oversub = b->n_worlds > b->resident_waves;
  int n_chunks = 1;
  b->st.n_chunks = 1; b->st.csched = b->csched_buf; b->st.handoff = b->handoff_buf; b->st.handoff_stride = b->handoff_stride;
  if (oversub && b->chunking && b->csched_buf && b->handoff_buf && n_steps >= 2 * b->min_chunk_steps) {
    int start = 0, c = 0;
    while (start < n_steps && c < b->max_chunks) {
      // (the library's own plan — no chunk_div option given: launches of more than 64 steps halve; on flat ground with a leg-chain
      // skeleton launches of up to 30 steps take 1.6 instead of 1.7 — 20 steps = 13 + 5 + 2, three chunks instead of 12 + 5 + 2 + 1:
      // 60.05 -> 60.6 M at the driver's arguments, round 6; 30 steps tie, 40 and 50 steps keep 1.7: 63.0 against 62.5 M)
      const double div = !b->chunk_div_short ? b->chunk_div : n_steps > 64 ? 2.0 : (b->chunk_div < 1.75 && n_steps <= 30 ? 1.6 : b->chunk_div);
      int len = (int)std::ceil((n_steps - start) / div);
      len = std::max(len, b->min_chunk_steps);
      if (c == b->max_chunks - 1 || n_steps - start - len < b->min_chunk_steps) len = n_steps - start;
      b->st.chunk_start[c++] = start;
      start += len;
    }
    b->st.chunk_start[c] = n_steps;
    n_chunks = c;
    b->st.n_chunks = c;
  }
  b->st.sched_mode = n_chunks > 1 ? 1 : 0;
  // chunked: one persistent workgroup per resident wave pulls (chunk, world) items; plain: one workgroup per world
  dim3 grid(n_chunks > 1 ? (unsigned)std::min(b->resident_waves, b->n_worlds * n_chunks) : (unsigned)b->n_worlds), block(nmf::kWave);
  // more worlds than resident waves: the launch runs in rounds; the measured policy picks the world order (nmf_order_kernel)
  b->st.order = nullptr; b->st.sched = nullptr;
  if (oversub && b->order_buf && b->sched_buf && b->order_policy != 2) {
    const int policy = b->order_policy == 3 ? (n_steps <= 64 ? 1 : -1) : b->order_policy;
    if (!(policy == 1 && b->order_valid && ++b->order_age < b->order_every)) {
      hipLaunchKernelGGL(nmf::nmf_order_kernel, dim3(1), dim3(1024), 0, stream, b->st.cost, b->n_worlds, b->order_buf, b->sched_buf, n_steps, policy);
      b->order_age = 0; b->order_valid = true;
    }
    b->st.order = b->order_buf;
    if (policy < 0) b->st.sched = b->sched_buf;
  }
  // the batch's stepping kernel (step_kernel): nmf_step_kernel(const DevModel*, DevState, ReplayArgs, int)
  const nmf::DevModel* dm = b->dm_dev;
  nmf::ReplayArgs rp_arg = rp;
  void* args[] = {&dm, &b->st, &rp_arg, &n_steps};
  (void)hipLaunchKernel(b->step_fn, grid, block, args, b->lds_pad, stream);
  HIP_OK(hipGetLastError());
  return 0;
}

// Development overrides from the process environment — honoured only under NMF_ALLOW_ENV=1 (the one getenv gate of this
// library): a stray NMF_* variable in a user's shell never changes what a batch runs.
const char* dev_env(const char* name) {
  static const bool allowed = [] { const char* e = getenv("NMF_ALLOW_ENV"); return e && atoi(e) != 0; }();
  return allowed ? getenv(name) : nullptr;
}

// nmf_batch_options (0 = the library's default) with the development overrides written over it: an override beats an option.
// chunk_div is a double (the override's precision) and 0 unless given: an option <= 1 is no request, an override >= 1 is one.
struct Options {
  int solver = 0, sched = 0, order = 0, max_chunks = 0, min_chunk_steps = 0, order_every = 0, rest_slow = 0, flies_per_cu = 0;
  double chunk_div = 0.0;
};

Options read_options(const nmf_batch_options& in) {
  Options o;
  o.solver = in.solver; o.sched = in.sched; o.order = in.order; o.max_chunks = in.max_chunks; o.min_chunk_steps = in.min_chunk_steps;
  o.order_every = in.order_every; o.rest_slow = in.rest_slow; o.flies_per_cu = in.flies_per_cu;
  if (in.chunk_div > 1.f) o.chunk_div = in.chunk_div;
  // NMF_SOLVER = primal | nohist | nofallback (default: contact-space solve with the active-set history); NMF_SCHED = chunks
  // (default) | plain; NMF_ORDER = auto (default) | inorder | costliest | none | policy (the option codes of include/nmf.h)
  if (const char* e = dev_env("NMF_SOLVER")) {
    const std::string v(e);
    o.solver = v == "primal" ? 1 : v == "nohist" ? 2 : v == "nofallback" ? 4 : 0;
  }
  if (const char* e = dev_env("NMF_SCHED")) o.sched = std::string(e) == "plain" ? 1 : 0;
  if (const char* e = dev_env("NMF_ORDER")) {
    const std::string v(e);
    o.order = v == "inorder" ? 1 : v == "costliest" ? 2 : v == "none" ? 3 : v == "policy" ? 4 : 0;
  }
  if (const char* e = dev_env("NMF_ORDER_EVERY")) o.order_every = std::max(1, atoi(e));
  if (const char* e = dev_env("NMF_MAX_CHUNKS")) o.max_chunks = std::max(1, std::min(16, atoi(e)));
  if (const char* e = dev_env("NMF_CHUNK_DIV")) o.chunk_div = std::max(1.0, atof(e));
  if (const char* e = dev_env("NMF_MIN_CHUNK_STEPS")) o.min_chunk_steps = std::max(1, atoi(e));
  if (const char* e = dev_env("NMF_FLIES_PER_CU")) o.flies_per_cu = atoi(e);
  // NMF_DISABLE_REST_FAST: diagnostic switch, forces the table-driven level passes (tests cover both paths)
  if (dev_env("NMF_DISABLE_REST_FAST")) o.rest_slow = 1;
  return o;
}

// DevModel: the model's scalars and arrays, the tree tables and the solver option bits, uploaded to b->dm_dev
int fill_model(nmf_batch* b, const Skeleton& sk, const Options& opt) {
  const nmf_model* model = b->model;
  const nmf::Family& fam = nmf::family(sk.topo);
  const std::vector<int> &tree_body = sk.tree_body, &child_start = sk.child_start, &child_count = sk.child_count, &lvl_start = sk.lvl_start;
  nmf::DevModel& d = b->dm;
  d.nb = model->nb; d.nv = model->nv; d.nq = model->nq; d.nu = model->nu; d.ng = model->ng;
  d.nseg = model->nseg; d.nsite = model->nsite; d.nsensor = model->nsensor; d.max_iter = model->max_iter;
  auto scalar = [&](const char* nm, int k) { const HostArray* a = model->find(nm); return a && !a->is_int && (int)a->f.size() > k ? a->f[(size_t)k] : 0.f; };
  d.timestep = scalar("opt_timestep", 0); d.tolerance = scalar("opt_tolerance", 0);
  d.hull_skin = scalar("hull_skin", 0); d.meaninertia = scalar("stat_meaninertia", 0);
  for (int k = 0; k < 3; ++k) d.gravity[k] = scalar("opt_gravity", k);
  for (int k = 0; k < 4; ++k) d.plane[k] = scalar("plane", k);
  for (int k = 0; k < 5; ++k) d.terrain[k] = scalar("terrain_params", k);
  { const HostArray* wa = model->find("weld_active"); d.weld_active = wa && wa->is_int && !wa->i.empty() ? wa->i[0] : 0;
    for (int k = 0; k < 3; ++k) d.weld_pos[k] = scalar("weld_params", k);
    for (int k = 0; k < 4; ++k) d.weld_quat[k] = scalar("weld_params", 3 + k);
    for (int k = 0; k < 2; ++k) d.weld_solref[k] = scalar("weld_params", 7 + k);
    for (int k = 0; k < 5; ++k) d.weld_solimp[k] = scalar("weld_params", 9 + k);
    for (int k = 0; k < 2; ++k) d.weld_invweight[k] = scalar("weld_params", 14 + k); }
  { const HostArray* so = model->find("sem_options");
    if (!so || !so->is_int || so->i.size() < 5) return fail("nmf_batch_create: model lacks sem_options");
    d.sem_terrain_walls = so->i[4];
    d.sem_pyramid_plain = so->i[0]; d.sem_adhesion_fused = so->i[1]; d.sem_sensor_contact_frame = so->i[2];
    d.sem_max_hull_contacts = so->i[3] >= 1 && so->i[3] <= 4 ? so->i[3] : 4; }
  { const HostArray* tt = model->find("terrain_type"); d.terrain_type = tt && tt->is_int && !tt->i.empty() ? tt->i[0] : 0; }
  int rc = 0;
#define UF(n) rc |= upload_f(b, #n, (void*)&d.n)
#define UI(n) rc |= upload_i(b, #n, (void*)&d.n)
  UF(body_pos); UF(body_quat); UF(body_mass); UF(body_ipos); UF(body_inertia);
  UI(body_dofadr); UI(body_dofnum); UI(dof_body);
  UF(dof_axis); UF(dof_armature); UF(dof_damping); UF(dof_stiffness); UF(dof_springref);
  UI(seg_body); UF(seg_pos); UF(seg_quat); UI(site_body); UF(site_pos);
  UI(act_type); UI(act_trn); UI(act_limited); UI(act_geom); UF(act_gain); UF(act_bias); UF(act_forcerange); UF(act_ctrlrange);
  UF(key_qpos); UF(key_ctrl);
  d.act_general = nullptr;
  if (const HostArray* ag = model->find("act_general")) {        // optional: models with intvelocity / damper / cylinder / muscle actuators or shared dofs
    if (ag->is_int || (int)ag->f.size() != model->nu * nmf::kActGen) { rc |= fail("nmf_batch_create: act_general must be float [nu][32]"); }
    else {
      UF(act_general);
      // the affine pass of the stepping kernel writes every actuator's force to its dof with a plain store (one lane per actuator,
      // one actuator per dof): the general actuators' zero force goes to dof 0 — no affine actuator drives the root — instead of
      // racing with the affine actuator that may share their dof; the general pass reads the dof from the row's flags
      std::vector<int> trn = model->find("act_trn")->i;
      for (int u = 0; u < model->nu; ++u) if ((int)ag->f[(size_t)u * nmf::kActGen] & 1) trn[(size_t)u] = 0;
      upload(b, trn, &d.act_trn);
    }
  }
  UI(geom_body); UI(geom_type); UI(geom_hulladr); UI(geom_hullnum); UI(geom_sensor);
  UF(geom_p0); UF(geom_p1); UF(geom_radius); UF(geom_bsphere); UF(geom_invweight0); UF(hull_vert);
  UF(pair_friction); UF(pair_solref); UF(pair_solimp); UF(pair_margin);
#undef UF
#undef UI
  if (fam.tree_tables()) {
    const HostArray* bp = model->find("body_parent");
    upload(b, bp->i, &d.body_parent);
    upload(b, tree_body, &d.tree_body);
    upload(b, child_start, &d.tree_child_start);
    upload(b, child_count, &d.tree_child_count);
    d.tree_nlevel = (int)lvl_start.size() - 1;
    for (size_t k = 0; k < 18; ++k) d.tree_lvl_start[k] = k < lvl_start.size() ? lvl_start[k] : (int)tree_body.size();
    d.rest_fast = 0; d.rest_pack = nullptr;
    std::vector<int> pack;
    if (fam.hybrid() && !opt.rest_slow && rest_pack_words(model, sk, pack)) { d.rest_fast = 1; upload(b, pack, &d.rest_pack); }
  } else {
    d.body_parent = d.tree_body = d.tree_child_start = d.tree_child_count = nullptr; d.tree_nlevel = 0; d.rest_fast = 0; d.rest_pack = nullptr;
  }
  d.noslip_iter = 0;
  if (const HostArray* os2 = model->find("opt_solver")) { if (os2->i.size() > 1) d.noslip_iter = os2->i[1]; }
  d.max_contacts = nmf::kMaxCon;
  d.solver_flags = opt.solver & 7;
  if (rc != 0) return rc;
  b->dm_dev = (nmf::DevModel*)b->mem.upload(&d, sizeof(nmf::DevModel));
  return b->mem.ok ? 0 : -1;
}

// DevState: the per-world fields and the stepping kernel's scratch
int alloc_state(nmf_batch* b) {
  const nmf_model* model = b->model;
  const size_t n_worlds = (size_t)b->n_worlds;
  nmf::DevState& st = b->st;
  st.n_worlds = b->n_worlds;
  float* stats_sum = nullptr;
  b->handoff_stride = (model->nq + 2 * model->nv + model->nu + 6 + nmf::kActHistWords + 63) / 64 * 64;      // state, controls, clock + 5 running sums, active-set history
  alloc_field(b, NMF_QPOS, model->nq, &st.qpos); alloc_field(b, NMF_QVEL, model->nv, &st.qvel);
  alloc_field(b, NMF_CTRL, model->nu, &st.ctrl); alloc_field(b, NMF_QACC_WARMSTART, model->nv, &st.qacc_ws);
  alloc_field(b, NMF_SEG_XPOS, model->nseg * 3, &st.seg_xpos); alloc_field(b, NMF_SEG_XQUAT, model->nseg * 4, &st.seg_xquat);
  alloc_field(b, NMF_SITE_XPOS, model->nsite * 3, &st.site_xpos); alloc_field(b, NMF_ACTUATOR_FORCE, model->nu, &st.actuator_force);
  alloc_field(b, NMF_SENSORDATA, 96, &st.sensordata); alloc_field(b, NMF_TIME, 1, &st.time);
  alloc_field(b, NMF_STATS, 8, &st.stats); alloc_field(b, NMF_QACC, model->nv, &st.qacc); alloc_field(b, NMF_COST, 1, &st.cost);
  alloc_field(b, NMF_STATS_SUM, 16, &stats_sum);        // uint32 counters
  alloc_field(b, NMF_CONTACT_GEOM, nmf::kMaxCon, &st.contact_geom); alloc_field(b, NMF_ACT, model->nu, &st.act);
  alloc_dev(b, n_worlds, &b->order_buf); alloc_dev(b, 1, &b->csched_buf);
  alloc_dev(b, n_worlds * (size_t)b->handoff_stride, &b->handoff_buf);      // tag 0 = no launch's
  alloc_dev(b, n_worlds * nmf::kActHistWords, &st.act_hist);
  st.stats_sum = reinterpret_cast<unsigned int*>(stats_sum);
  st.dual_scratch = nullptr;
  // kDualGlob (ALL_POSSIBLE): the contact-space solve's leg factors live in HBM, one block per workgroup of a launch (<= n_worlds)
  // kEulerFused (leg-chain kernels): Euler's factors, written by the smooth solve of the same step, likewise
  with_topo(b->topo, [&](auto tag) {
    using TP = typename decltype(tag)::type;
    if (nmf::kDualGlob<TP>) alloc_dev(b, n_worlds * nmf::kDualScratchFloats, &st.dual_scratch);
    else if (nmf::kEulerFused<TP>) alloc_dev(b, n_worlds * (size_t)nmf::euler_scratch_floats<TP>(), &st.dual_scratch);
  });
  st.noslip_buf = nullptr;
  // CPU flavour: scratch of the primal path's noslip pass (157 KB per world)
  if (b->dm.noslip_iter > 0) alloc_dev(b, n_worlds * nmf::kNoslipFloats, &st.noslip_buf);
  alloc_dev(b, 2, &b->clock_probe_buf); alloc_dev(b, 1, &b->sched_buf);
  st.clock_probe = b->clock_probe_buf;
  st.sched = nullptr;
  st.order = nullptr;
  return b->mem.ok ? 0 : -1;
}

// The chunk plan and the world order of launch()
void set_schedule(nmf_batch* b, const Options& opt) {
  b->chunking = opt.sched != 1;
  if (opt.order) b->order_policy = opt.order == 1 ? 0 : opt.order == 2 ? 1 : opt.order == 3 ? 2 : opt.order == 4 ? -1 : 3;
  if (opt.order_every > 0) b->order_every = opt.order_every;
  if (opt.max_chunks > 0) b->max_chunks = std::max(1, std::min(16, opt.max_chunks));
  // (the family's own divisor on flat ground — NMF_FAMILIES, nmf_families.h —, halving chunks over a terrain)
  b->chunk_div = b->dm.terrain_type == 0 ? nmf::family(b->topo).chunk_div : 2.0;
  b->chunk_div_short = true;
  if (opt.chunk_div > 0.0) { b->chunk_div = opt.chunk_div; b->chunk_div_short = false; }
  if (opt.min_chunk_steps > 0) b->min_chunk_steps = opt.min_chunk_steps;
  // (activations live in HBM and are advanced in place every step by the lane that owns the actuator: a world's steps must stay
  // on one workgroup within a launch — whole-launch work items for the models that have general actuators)
  if (b->dm.act_general) b->chunking = false;
}

// The stepping kernel and its residency: flies (= single-wave workgroups) a CU holds at once, asked of the runtime for the
// kernel this batch will launch (LDS- or register-limited, whichever binds); fallback = the family's figure in NMF_FAMILIES
int pick_kernel(nmf_batch* b, const Options& opt) {
  const int topo = b->topo, device = b->mem.device;
  int per_cu = nmf::family(topo).per_cu;
  const bool weld = b->dm.weld_active != 0, terrain = b->dm.terrain_type != 0;
  if (weld && terrain) return fail("nmf_batch_create: a tethered world has no terrain");
  const void* fn = step_kernel(topo, weld, terrain);
  if (!fn) return fail("nmf_batch_create: this build of the library has no kernel for the model's skeleton (NMF_TOPO_MASK)");
  int nblk = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nblk, fn, nmf::kWave, 0) == hipSuccess && nblk > 0) per_cu = nblk;
  b->step_fn = fn;
  // options.flies_per_cu below the kernel's own residency: idle LDS per workgroup so that k workgroups fit a CU and k + 1 do
  // not — as little of it as that takes (allocation granule 512 B), so the CU keeps LDS for another stream's kernel
  const int want = opt.flies_per_cu;
  hipFuncAttributes fa;
  if (want > 0 && want < per_cu && hipFuncGetAttributes(&fa, fn) == hipSuccess) {
    int lds_cu = 0;
    if (hipDeviceGetAttribute(&lds_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, device) != hipSuccess || lds_cu <= 0) lds_cu = 160 * 1024;
    const int granule = 512;
    int per_wg = (lds_cu / (want + 1) / granule + 1) * granule;            // the smallest allocation of which want + 1 do not fit
    if (per_wg * want <= lds_cu && per_wg > (int)fa.sharedSizeBytes) {
      b->lds_pad = (unsigned)(per_wg - (int)fa.sharedSizeBytes);
      int nblk2 = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nblk2, fn, nmf::kWave, b->lds_pad) == hipSuccess && nblk2 > 0) per_cu = std::min(per_cu, nblk2);
      else per_cu = want;
    }
  }
  if (const char* e = dev_env("NMF_LDS_PAD")) b->lds_pad = (unsigned)atoi(e);
  b->per_cu = per_cu;
  hipDeviceProp_t prop;
  b->resident_waves = (hipGetDeviceProperties(&prop, device) == hipSuccess ? prop.multiProcessorCount : 256) * per_cu;
  return 0;
}

}  // namespace

extern "C" nmf_batch* nmf_batch_create(const nmf_model* model, int n_worlds, int device) {
  return nmf_batch_create_ex(model, n_worlds, device, nullptr);
}

extern "C" nmf_batch* nmf_batch_create_ex(const nmf_model* model, int n_worlds, int device, const nmf_batch_options* options) {
  g_err.clear();
  nmf_batch_options in{};
  if (options) {
    if (options->struct_size < (int32_t)sizeof(int32_t) || options->struct_size > (int32_t)sizeof(nmf_batch_options)) { fail("nmf_batch_create_ex: options->struct_size does not match this library"); return nullptr; }
    memcpy(&in, options, (size_t)options->struct_size);
  }
  if (!model) { fail("nmf_batch_create: null model"); return nullptr; }
  if (n_worlds <= 0) { fail("nmf_batch_create: n_worlds must be positive"); return nullptr; }
  Skeleton sk;
  if (const char* why = classify_skeleton(model, sk)) { fail(why); return nullptr; }
  DeviceGuard guard(device);            // allocations and the first reset run on `device`; the caller's device comes back on return
  if (guard.err != hipSuccess) { fail("nmf_batch_create: hipSetDevice failed (no MI355X visible?)"); return nullptr; }
  const Options opt = read_options(in);
  auto* b = new nmf_batch();
  b->model = model; b->n_worlds = n_worlds; b->topo = sk.topo;
  b->mem.device = device; b->mem.who = "nmf_batch_create";
  if (fill_model(b, sk, opt) != 0 || alloc_state(b) != 0 || (set_schedule(b, opt), pick_kernel(b, opt)) != 0 ||
      nmf_reset(b, nullptr) != 0 || hipDeviceSynchronize() != hipSuccess) {
    const std::string keep = g_err.empty() ? std::string("nmf_batch_create: device initialisation failed") : g_err;
    nmf_batch_destroy(b);
    g_err = keep;
    return nullptr;
  }
  return b;
}

extern "C" void nmf_batch_destroy(nmf_batch* b) {
  if (!b) return;
  b->mem.release();
  for (nmf_eye_plan* q : b->eye_plans) nmf_eye_plan_destroy(q);
  delete b;
}

extern "C" int nmf_batch_n_worlds(const nmf_batch* b) { return b ? b->n_worlds : 0; }

extern "C" int nmf_batch_info(const nmf_batch* b, int32_t out[16]) {
  if (!b || !out) return fail("nmf_batch_info: null argument");
  const bool weld = b->dm.weld_active != 0, terrain = b->dm.terrain_type != 0;
  int flavour = 0, maxcon = 0;
  with_topo(b->topo, [&](auto tag) {      // the general-tree families have neither flavour (kDualS, kDualH false)
    using TP = typename decltype(tag)::type;
    if (!weld && !(b->dm.solver_flags & 1)) { flavour = nmf::kDualS<TP> ? 1 : nmf::kDualH<TP> ? 2 : 0; maxcon = flavour ? nmf::kDualMaxCon<TP> : 0; }
  });
  out[0] = b->topo; out[1] = terrain ? 1 : 0; out[2] = weld ? 1 : 0; out[3] = flavour; out[4] = maxcon;
  out[5] = b->per_cu; out[6] = b->resident_waves; out[7] = b->chunking ? 1 : 0; out[8] = b->max_chunks;
  out[9] = (int32_t)std::lround(1000.0 * b->chunk_div); out[10] = b->order_policy; out[11] = b->dm.solver_flags;
  out[12] = b->dm.noslip_iter; out[13] = b->dm.max_contacts; out[14] = 0; out[15] = 0;
  hipFuncAttributes fa;
  if (b->step_fn && hipFuncGetAttributes(&fa, b->step_fn) == hipSuccess) { out[14] = (int32_t)fa.sharedSizeBytes; out[15] = fa.numRegs; }
  return 0;
}

extern "C" int nmf_reset(nmf_batch* b, void* stream) {
  if (!b) return fail("nmf_reset: null batch");
  b->steps = 0;
  return launch_reset(b, nullptr, (hipStream_t)stream);
}

extern "C" int nmf_reset_worlds(nmf_batch* b, const uint8_t* mask_dev, void* stream) {
  if (!b) return fail("nmf_reset_worlds: null batch");
  if (!mask_dev) return fail("nmf_reset_worlds: null mask");
  return launch_reset(b, mask_dev, (hipStream_t)stream);
}

extern "C" int nmf_step(nmf_batch* b, int n_steps, void* stream) {
  if (!b) return fail("nmf_step: null batch");
  if (n_steps <= 0) return fail("nmf_step: n_steps must be positive");
  nmf::ReplayArgs rp{nullptr, nullptr, 1, 0, 0};
  b->steps += n_steps;
  return launch(b, rp, n_steps, (hipStream_t)stream);
}

extern "C" int nmf_step_replay(nmf_batch* b, const float* table_dev, int table_steps, int n_act,
                               const int32_t* act_ids_dev, int start, int n_steps, void* stream) {
  if (!b) return fail("nmf_step_replay: null batch");
  if (n_steps <= 0) return fail("nmf_step_replay: n_steps must be positive");
  if (!table_dev || !act_ids_dev || table_steps <= 0 || n_act <= 0 || n_act > b->model->nu)
    return fail("nmf_step_replay: bad replay table arguments");
  nmf::ReplayArgs rp{table_dev, act_ids_dev, table_steps, n_act, ((start % table_steps) + table_steps) % table_steps};
  b->steps += n_steps;
  return launch(b, rp, n_steps, (hipStream_t)stream);
}

extern "C" int nmf_step_record(nmf_batch* b, const float* table_dev, int table_steps, int n_act_table, const int32_t* act_ids_dev, int start,
                               int n_steps, int obs_every, int n_joint, int n_act, float* ring_dev, int row_stride, void* stream) {
  if (!b) return fail("nmf_step_record: null batch");
  if (n_steps <= 0 || obs_every <= 0) return fail("nmf_step_record: n_steps and obs_every must be positive");
  if (n_steps % obs_every) return fail("nmf_step_record: n_steps must be a multiple of obs_every (the trailing steps would not be recorded)");
  if (!ring_dev) return fail("nmf_step_record: null ring");
  const nmf_model* m = b->model;
  if (n_joint < 0 || n_joint > m->nv - 6 || n_act < 0 || n_act > m->nu || row_stride < 2 * n_joint + n_act + 96)
    return fail("nmf_step_record: need 0 <= n_joint <= nv - 6, 0 <= n_act <= nu and row_stride >= 2 n_joint + n_act + 96");
  nmf::ReplayArgs rp{nullptr, nullptr, 1, 0, 0};
  if (table_dev) {
    if (!act_ids_dev || table_steps <= 0 || n_act_table <= 0 || n_act_table > m->nu) return fail("nmf_step_record: bad replay table arguments");
    rp = nmf::ReplayArgs{table_dev, act_ids_dev, table_steps, n_act_table, ((start % table_steps) + table_steps) % table_steps};
  }
  RingArgs ring;
  ring.ring = ring_dev; ring.stride = row_stride; ring.every = obs_every; ring.nj = n_joint; ring.nact = n_act;
  b->steps += n_steps;
  return launch(b, rp, n_steps, (hipStream_t)stream, ring);
}

extern "C" float* nmf_field_ptr(nmf_batch* b, int field, int32_t* width) {
  if (!b || field < 0 || field >= NMF_FIELD_COUNT) { fail("nmf_field_ptr: bad field"); return nullptr; }
  if (width) *width = b->widths[field];
  return b->fields[field];
}

extern "C" int nmf_gather(nmf_batch* b, int field, const int32_t* ids_dev, int n_ids, int group, float* dst_dev, void* stream) {
  if (!b || field < 0 || field >= NMF_FIELD_COUNT) return fail("nmf_gather: bad field");
  if (n_ids <= 0) return 0;
  if (group < 1 || !ids_dev || !dst_dev) return fail("nmf_gather: bad arguments");
  DEVICE_GUARD(b);
  size_t total = (size_t)b->n_worlds * n_ids * group;
  int blocks = (int)((total + 255) / 256); if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(nmf::nmf_gather_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, b->fields[field],
                     b->widths[field], ids_dev, n_ids, group, dst_dev, b->n_worlds);
  HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int nmf_scatter(nmf_batch* b, int field, const int32_t* ids_dev, int n_ids, const float* src_dev, void* stream) {
  if (!b || field < 0 || field >= NMF_FIELD_COUNT) return fail("nmf_scatter: bad field");
  if (n_ids <= 0) return 0;
  if (!ids_dev || !src_dev) return fail("nmf_scatter: bad arguments");
  DEVICE_GUARD(b);
  size_t total = (size_t)b->n_worlds * n_ids;
  int blocks = (int)((total + 255) / 256); if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(nmf::nmf_scatter_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, b->fields[field],
                     b->widths[field], ids_dev, n_ids, src_dev, b->n_worlds);
  HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int nmf_pack_observations(nmf_batch* b, int n_joint, int n_act, float* out_dev, int row_stride, void* stream) {
  if (!b || !out_dev) return fail("nmf_pack_observations: null argument");
  const nmf_model* m = b->model;
  const int width = 2 * n_joint + n_act + 96;
  if (n_joint < 0 || n_joint > m->nv - 6 || n_act < 0 || n_act > m->nu || row_stride < width)
    return fail("nmf_pack_observations: need 0 <= n_joint <= nv - 6, 0 <= n_act <= nu and row_stride >= 2 n_joint + n_act + 96");
  DEVICE_GUARD(b);
  const size_t total = (size_t)b->n_worlds * width;
  int blocks = (int)((total + 255) / 256); if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(nmf::nmf_pack_obs_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, b->st.qpos, b->st.qvel,
                     b->st.actuator_force, b->st.sensordata, m->nq, m->nv, m->nu, n_joint, n_act, b->n_worlds, out_dev, row_stride);
  HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int64_t nmf_step_count(const nmf_batch* b) { return b ? b->steps : 0; }

extern "C" int nmf_shader_clock(nmf_batch* b, double* hz_out, int reset) {
  if (!b || !hz_out) return fail("nmf_shader_clock: null argument");
  DEVICE_GUARD(b);
  unsigned long long v[2] = {0, 0};
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(v, b->clock_probe_buf, sizeof(v), hipMemcpyDeviceToHost));
  *hz_out = v[1] ? 1e8 * (double)v[0] / (double)v[1] : 0.0;
  if (reset) HIP_OK(hipMemset(b->clock_probe_buf, 0, sizeof(v)));
  return 0;
}

extern "C" double nmf_time_launches(nmf_batch* b, const float* table_dev, int table_steps, int n_act,
                                    const int32_t* act_ids_dev, int n_steps, int reps, void* stream) {
  if (!b || reps <= 0 || n_steps <= 0) { fail("nmf_time_launches: bad arguments"); return -1.0; }
  hipStream_t s = (hipStream_t)stream;
  hipEvent_t e0, e1;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { fail("hipEventCreate failed"); return -1.0; }
  (void)hipEventRecord(e0, s);
  int start = 0;
  for (int r = 0; r < reps; ++r) {
    int rc = table_dev ? nmf_step_replay(b, table_dev, table_steps, n_act, act_ids_dev, start, n_steps, stream)
                       : nmf_step(b, n_steps, stream);
    if (rc != 0) { (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); return -1.0; }
    start += n_steps;
  }
  (void)hipEventRecord(e1, s);
  if (hipEventSynchronize(e1) != hipSuccess) { fail("hipEventSynchronize failed"); return -1.0; }
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  return (double)ms / reps;
}

extern "C" size_t nmf_retina_plan_bytes(int n_pixels) {
  if (n_pixels <= 0 || n_pixels % 16) return 0;
  const size_t n_chunk = (size_t)n_pixels / 16;
  return n_chunk * 16 + ((n_chunk * 4 + 4 + 15) / 16) * 16;
}

extern "C" int nmf_retina_plan(const int16_t* id_map_dev, int n_pixels, void* plan_dev, void* stream) {
  if (!id_map_dev || !plan_dev) return fail("nmf_retina_plan: null buffer");
  if (n_pixels <= 0 || n_pixels % 16) return fail("nmf_retina_plan: n_pixels must be a positive multiple of 16");
  if (reinterpret_cast<uintptr_t>(plan_dev) & 15u) return fail("nmf_retina_plan: plan must be 16-byte aligned");
  const int n_chunk = n_pixels / 16;
  hipLaunchKernelGGL(nmf::nmf_retina_plan_kernel, dim3((unsigned)((n_chunk + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     id_map_dev, n_chunk, reinterpret_cast<nmf::u32x4*>(plan_dev));
  hipLaunchKernelGGL(nmf::nmf_retina_active_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, id_map_dev, n_chunk,
                     reinterpret_cast<int*>(static_cast<char*>(plan_dev) + (size_t)n_chunk * 16));
  HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int nmf_retina_resample(const uint8_t* images_dev, const int16_t* id_map_dev, const void* plan_dev,
                                   const uint8_t* pale_dev, const float* inv_norm_dev, int n_images, int n_pixels,
                                   int n_ommatidia, float* out_dev, void* stream) {
  if (!images_dev || !id_map_dev || !pale_dev || !inv_norm_dev || !out_dev) return fail("nmf_retina_resample: null buffer");
  if (n_images <= 0) return 0;
  if (n_pixels <= 0 || n_ommatidia <= 0 || n_ommatidia > nmf::kMaxOmmatidia)
    return fail("nmf_retina_resample: need 0 < n_ommatidia <= 1024 and n_pixels > 0");
  if ((reinterpret_cast<uintptr_t>(images_dev) | reinterpret_cast<uintptr_t>(id_map_dev) | reinterpret_cast<uintptr_t>(plan_dev)) & 15u ||
      (n_pixels * 3) % 16)
    return fail("nmf_retina_resample: images / id map / plan must be 16-byte aligned and image size a multiple of 16 bytes");
  if (plan_dev && n_pixels % 1024 == 0)
    hipLaunchKernelGGL(nmf::nmf_retina_stream_kernel, dim3((unsigned)n_images), dim3(nmf::kRetinaThreads), 0, (hipStream_t)stream,
                       images_dev, id_map_dev, reinterpret_cast<const nmf::u32x4*>(plan_dev), pale_dev, inv_norm_dev, n_pixels,
                       n_ommatidia, out_dev);
  else
    hipLaunchKernelGGL(nmf::nmf_retina_kernel, dim3((unsigned)n_images), dim3(nmf::kRetinaThreads), 0, (hipStream_t)stream,
                       images_dev, id_map_dev, pale_dev, inv_norm_dev, n_pixels, n_ommatidia, out_dev);
  HIP_OK(hipGetLastError());
  return 0;
}

extern "C" size_t nmf_eye_params_size(void) { return sizeof(nmf_eye_params); }

// Visit plan of the eye renderer: the chunks (16 consecutive raw pixels) to render, sorted by 32 x 32-pixel tile and cut
// into groups of 64 (one wave's turn), each group with the bounding cone of its rays in the camera frame (axis, cos and
// sin of the half-angle) — so that a wave can decide per group what it can see at all.  Built on the host once per id map.
extern "C" void nmf_eye_plan_destroy(nmf_eye_plan* P) {
  if (!P) return;
  P->mem.release();
  delete P;
}

// NOT stream-ordered: device-to-host copies of the id map / run plan / pale flags, host-side sorting, allocations and uploads — once
// per (id map, lens, ommatidia types).  Every failure path gives back what was allocated (nmf_eye_plan_destroy).
static int fill_eye_plan(nmf_eye_plan* Pp, const int16_t* id_map_dev, const void* plan_dev, const uint8_t* pale_dev, const float* inv_norm_dev, int h, int w, float fov_deg, int n_omm) {
  nmf_eye_plan& P = *Pp;
  const int n_pix = h * w, n_chunk = n_pix / 16;
  std::vector<int16_t> ids((size_t)n_pix);
  HIP_OK(hipMemcpy(ids.data(), id_map_dev, sizeof(int16_t) * (size_t)n_pix, hipMemcpyDeviceToHost));
  const double half_fov = 0.5 * fov_deg * 3.14159265358979323846 / 180.0, inv_half_h = 2.0 / h, cx = 0.5 * w, cy = 0.5 * h;
  std::vector<double> ray((size_t)n_pix * 3);
  for (int i = 0; i < n_pix; ++i) {
    const int row = i / w, col = i - row * w;
    const double u = (col + 0.5 - cx) * inv_half_h, v = (row + 0.5 - cy) * inv_half_h;
    const double rho = std::sqrt(std::max(u * u + v * v, 1e-24)), th = rho * half_fov;
    ray[3 * (size_t)i] = std::sin(th) * u / rho; ray[3 * (size_t)i + 1] = -std::sin(th) * v / rho; ray[3 * (size_t)i + 2] = -std::cos(th);
  }
  // bounding cone (axis, cos of the half-angle) of a set of pixels
  auto cone_of = [&](const std::vector<size_t>& px, double margin, float* out) {
    double ax = 0, ay = 0, az = 0;
    for (size_t i : px) { ax += ray[3 * i]; ay += ray[3 * i + 1]; az += ray[3 * i + 2]; }
    const double nrm = std::sqrt(ax * ax + ay * ay + az * az);
    if (px.empty() || nrm < 1e-9) { out[0] = 0.f; out[1] = 0.f; out[2] = -1.f; out[3] = px.empty() ? 1.f : -1.f; return; }   // nothing / everything
    ax /= nrm; ay /= nrm; az /= nrm;
    double cmin = 1.0;
    for (size_t i : px) cmin = std::min(cmin, ax * ray[3 * i] + ay * ray[3 * i + 1] + az * ray[3 * i + 2]);
    out[0] = (float)ax; out[1] = (float)ay; out[2] = (float)az; out[3] = (float)std::max(-1.0, cmin - margin);
  };
  bool lens_ok = true;
  for (int i = 0; i < n_pix; ++i) lens_ok = lens_ok && ray[3 * (size_t)i + 2] < -std::cos(2.1);
  for (int mode = 0; mode < 2; ++mode) {
    // chunks that stay inside one image row, by tile; the ones that wrap to the next row (their rays lie at both image
    // edges: no common cone) in groups of their own, with one cone per piece
    std::vector<int> plain, wrapped;
    for (int ch = 0; ch < n_chunk; ++ch) {
      bool on = mode == 1;
      for (int k = 0; k < 16 && !on; ++k) on = (ids[(size_t)ch * 16 + k] & 0x7fff) != 0;
      if (!on) continue;
      ((ch * 16) / w == (ch * 16 + 15) / w ? plain : wrapped).push_back(ch);
    }
    auto key = [&](int ch) { const int row = (ch * 16) / w, col = ch * 16 - row * w; return ((long long)(row / 32) << 40) | ((long long)(col / 32) << 28) | ((long long)row << 12) | col; };
    std::sort(plain.begin(), plain.end(), [&](int a, int c) { return key(a) < key(c); });
    const int g_plain = (int)((plain.size() + 63) / 64), g_wrapped = (int)((wrapped.size() + 63) / 64), n_groups = g_plain + g_wrapped;
    std::vector<int> visit((size_t)n_groups * 64, -1);
    std::copy(plain.begin(), plain.end(), visit.begin());
    std::copy(wrapped.begin(), wrapped.end(), visit.begin() + (size_t)g_plain * 64);
    // per group: [0..3] cone of piece 0, [4..7] cone of piece 1 (wrapped groups), [8] 1 = two pieces; per slot: two cones
    std::vector<float> cones((size_t)n_groups * 12, 0.f), ccones(visit.size() * 8, 0.f);
    for (int g = 0; g < n_groups; ++g) {
      std::vector<size_t> gp[2];
      for (int l = 0; l < 64; ++l) {
        const size_t sl = (size_t)g * 64 + l;
        const int ch = visit[sl];
        std::vector<size_t> cp[2];
        if (ch >= 0) {
          const int row0 = (ch * 16) / w;
          for (int k = 0; k < 16; ++k) { const size_t i = (size_t)ch * 16 + k; const int pc = (int)(i / w) == row0 ? 0 : 1; cp[pc].push_back(i); gp[pc].push_back(i); }
        }
        cone_of(cp[0], 1e-5, &ccones[8 * sl]); cone_of(cp[1], 1e-5, &ccones[8 * sl + 4]);
      }
      cone_of(gp[0], 1e-4, &cones[(size_t)g * 12]); cone_of(gp[1], 1e-4, &cones[(size_t)g * 12 + 4]);
      cones[(size_t)g * 12 + 8] = g >= g_plain ? 1.f : 0.f;
      cones[(size_t)g * 12 + 9] = lens_ok ? 1.f : 0.f;      // [9]: every ray of the IMAGE within the range of the kernel's lens polynomials
    }
    P.visit[mode] = (int*)P.mem.upload(visit.data(), sizeof(int) * visit.size());
    P.cones[mode] = (float*)P.mem.upload(cones.data(), sizeof(float) * cones.size());
    P.chunk_cones[mode] = (float*)P.mem.upload(ccones.data(), sizeof(float) * ccones.size());
    P.n_groups[mode] = n_groups;
  }
  {
    // Sampled mode (nmf_eye_params::rays_per_ommatidium = 16): per ommatidium i the pixels of its cell in raster order,
    // P_0 .. P_{n-1}, and of those the 16 at indices floor((2 j + 1) n / 32), j = 0..15 (oracle/sensors_oracle.py::
    // sampled_pixels).  One lane per ray, an ommatidium's 16 rays in one DPP row.  The ommatidia are visited in 64 x 64
    // pixel tiles of their cells' centres, 16 (a 4 x 4 patch of the lattice) to a group: one bounding cone and one culling
    // for the group's 256 rays.  slot_omm[s] = the ommatidium in slot s.
    // Both lists carry what a ray would otherwise look up behind them (the sampled kernel waits for memory, not for arithmetic:
    // three dependent round trips per turn were visit -> the chunk's plan word, slot -> ommatidium -> pale): a visit entry is the
    // pixel | bit 30 "its chunk lies inside one image row and has a run plan" (the lens-polynomial path of the pixel-exact
    // kernel, nmf_eyes.hip); a slot entry is the ommatidium | bit 30 "pale".
    constexpr int K = nmf::kEyeRays, S = nmf::kEyeSlots;
    std::vector<uint32_t> planw((size_t)n_chunk * 4);
    std::vector<uint8_t> pale_h((size_t)n_omm);
    HIP_OK(hipDeviceSynchronize());        // (the caller's run plan was built on a stream of its own)
    HIP_OK(hipMemcpy(planw.data(), plan_dev, sizeof(uint32_t) * planw.size(), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(pale_h.data(), pale_dev, pale_h.size(), hipMemcpyDeviceToHost));
    std::vector<std::vector<int>> cell((size_t)n_omm);
    for (int i = 0; i < n_pix; ++i) { const int id = ids[(size_t)i] & 0x7fff; if (id > 0 && id <= n_omm) cell[(size_t)id - 1].push_back(i); }
    std::vector<int> order((size_t)n_omm);
    std::vector<long long> keyv((size_t)n_omm);
    for (int o = 0; o < n_omm; ++o) {
      order[(size_t)o] = o;
      double r = 0, c = 0;
      for (int i : cell[(size_t)o]) { r += i / w; c += i % w; }
      const double n = std::max<size_t>(cell[(size_t)o].size(), 1);
      const int row = (int)(r / n), col = (int)(c / n);
      keyv[(size_t)o] = ((long long)(row / 64) << 40) | ((long long)(col / 64) << 28) | ((long long)row << 12) | col;
    }
    std::stable_sort(order.begin(), order.end(), [&](int a, int c) { return keyv[(size_t)a] < keyv[(size_t)c]; });
    const int n_groups = (n_omm + S - 1) / S;
    std::vector<int> visit((size_t)n_groups * S * K, -1), slots((size_t)n_groups * S, 0);
    for (int sl = 0; sl < n_omm; ++sl) {
      const int o = order[(size_t)sl];
      slots[(size_t)sl] = o | (pale_h[(size_t)o] ? (1 << 30) : 0);
      const long long n = (long long)cell[(size_t)o].size();
      for (int j = 0; j < K && n > 0; ++j) {
        const int px = cell[(size_t)o][(size_t)(((2 * j + 1) * n) / (2 * K))];
        const int pchunk = px >> 4;
        const bool one_row = (pchunk * 16) / w == (pchunk * 16 + 15) / w, planned = !(planw[(size_t)pchunk * 4 + 1] & 0x10000u);
        visit[(size_t)sl * K + j] = px | (one_row && planned ? (1 << 30) : 0);
      }
    }
    // ... and one cone per TURN (64 rays = four ommatidia): every ray tests all the capsules its culling lets through, so the
    // sampled kernel culls a second time per turn (`chunk_cones` of this mode: axis + cos of the half-angle, camera frame)
    std::vector<float> cones((size_t)n_groups * 12, 0.f), tcones((size_t)n_groups * (S / 4) * 4, 0.f);
    for (int g = 0; g < n_groups; ++g) {
      std::vector<size_t> gp;
      for (int l = 0; l < S * K; ++l) if (visit[(size_t)g * S * K + l] >= 0) gp.push_back((size_t)(visit[(size_t)g * S * K + l] & 0xffffff));
      cone_of(gp, 1e-4, &cones[(size_t)g * 12]);
      cones[(size_t)g * 12 + 9] = lens_ok ? 1.f : 0.f;
      for (int t = 0; t < S / 4; ++t) {
        std::vector<size_t> tp;
        for (int l = 64 * t; l < 64 * (t + 1); ++l) if (visit[(size_t)g * S * K + l] >= 0) tp.push_back((size_t)(visit[(size_t)g * S * K + l] & 0xffffff));
        cone_of(tp, 1e-4, &tcones[((size_t)g * (S / 4) + t) * 4]);
      }
    }
    P.visit[2] = (int*)P.mem.upload(visit.data(), sizeof(int) * visit.size());
    P.cones[2] = (float*)P.mem.upload(cones.data(), sizeof(float) * cones.size());
    P.chunk_cones[2] = (float*)P.mem.upload(tcones.data(), sizeof(float) * tcones.size());
    P.slot_omm = (int*)P.mem.upload(slots.data(), sizeof(int) * slots.size());
    P.n_groups[2] = n_groups;
  }
  // the plan's own copies of what the kernel reads from the caller's buffers
  {
    const size_t rbytes = nmf_retina_plan_bytes(n_pix);
    P.id_map = (int16_t*)P.mem.alloc(sizeof(int16_t) * (size_t)n_pix); P.rplan = P.mem.alloc(rbytes);
    P.pale = (uint8_t*)P.mem.alloc((size_t)n_omm); P.inv_norm = (float*)P.mem.alloc(sizeof(float) * (size_t)n_omm);
    if (!P.mem.ok) return -1;
    HIP_OK(hipMemcpy(P.id_map, id_map_dev, sizeof(int16_t) * (size_t)n_pix, hipMemcpyDeviceToDevice));
    HIP_OK(hipMemcpy(P.rplan, plan_dev, rbytes, hipMemcpyDeviceToDevice));
    HIP_OK(hipMemcpy(P.pale, pale_dev, (size_t)n_omm, hipMemcpyDeviceToDevice));
    HIP_OK(hipMemcpy(P.inv_norm, inv_norm_dev, sizeof(float) * (size_t)n_omm, hipMemcpyDeviceToDevice));
    HIP_OK(hipDeviceSynchronize());
  }
  P.h = h; P.w = w; P.fov = fov_deg; P.n_omm = n_omm;
  return 0;
}

extern "C" nmf_eye_plan* nmf_eye_plan_create(const int16_t* id_map_dev, const void* plan_dev, const uint8_t* pale_dev, const float* inv_norm_dev,
                                             int height, int width, float fov_deg, int n_ommatidia, int device) {
  if (!id_map_dev || !plan_dev || !pale_dev || !inv_norm_dev) { fail("nmf_eye_plan_create: id map, plan, pale and inv_norm are required"); return nullptr; }
  if (height <= 0 || width <= 0 || (height * width) % 16) { fail("nmf_eye_plan_create: height * width must be a positive multiple of 16"); return nullptr; }
  if (n_ommatidia <= 0 || n_ommatidia > nmf::kMaxOmmatidia) { fail("nmf_eye_plan_create: need 0 < n_ommatidia <= 1024"); return nullptr; }
  if (!(fov_deg > 0.f) || fov_deg > 360.f) { fail("nmf_eye_plan_create: bad field of view"); return nullptr; }
  if (reinterpret_cast<uintptr_t>(plan_dev) & 15u) { fail("nmf_eye_plan_create: the run plan must be 16-byte aligned"); return nullptr; }
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) { fail("nmf_eye_plan_create: no such device"); return nullptr; }
  return build_or_destroy(device, "nmf_eye_plan_create", new nmf_eye_plan(), nmf_eye_plan_destroy, [&](nmf_eye_plan* P) {
    return fill_eye_plan(P, id_map_dev, plan_dev, pale_dev, inv_norm_dev, height, width, fov_deg, n_ommatidia);
  });
}

// The scene part of a renderer's kernel arguments (nmf::EyeArgs, nmf::CamArgs; nmf_scene.h draws it) from its public parameters
// (nmf_eye_params, nmf_camera_params: the same field names): checker, ground height, spheres, the relief the physics of batch b
// collides with, and the rgb table — 0 sky, 1 / 2 ground, 3 terrain side wall, the spheres from `first_sphere` on (everything else of
// the table 0: the caller fills the slots between afterwards).  Each caller keeps its own checks and error texts.
template <class Args, class Params>
void fill_scene(Args& A, const Params& p, const nmf_batch* b, int first_sphere) {
  A.checker_size = p.checker_size; A.ground_z = b->dm.plane[3];
  A.n_spheres = p.n_spheres; A.sphere_stride = p.spheres_per_world ? 4 * p.n_spheres : 0;
  A.terrain_kind = p.terrain_relief ? b->dm.terrain_type : 0;
  for (int k = 0; k < 5; ++k) A.terrain[k] = b->dm.terrain[k];
  std::memset(A.rgb, 0, sizeof(A.rgb));          // (the kernels load a material as a whole word: the fourth bytes are 0)
  for (int c = 0; c < 3; ++c) {
    A.rgb[0][c] = p.sky_rgb[c]; A.rgb[1][c] = p.ground_rgb[0][c]; A.rgb[2][c] = p.ground_rgb[1][c]; A.rgb[3][c] = p.wall_rgb[c];
    for (int s = 0; s < nmf::kMaxSpheres; ++s) A.rgb[first_sphere + s][c] = p.sphere_rgb[s][c];
  }
}

// Pure stream-ordered work: argument checks on the host, one kernel launch.  Everything the kernel reads besides the batch's poses and
// the caller's sphere / capsule lists belongs to the plan.
extern "C" int nmf_eye_render_planned(nmf_batch* b, const nmf_eye_params* p, const nmf_eye_plan* plan, const float* spheres_dev,
                                      const int32_t* capsule_seg_dev, const float* capsule_geom_dev,
                                      uint8_t* frames_out_dev, float* omm_out_dev, void* stream) {
  if (!b || !p || !plan) return fail("nmf_eye_render: null batch / params / plan");
  if (plan->mem.device != b->mem.device) return fail("nmf_eye_render: the plan lives on another device than the batch");
  if (plan->h != p->height || plan->w != p->width || plan->fov != p->fov_deg) return fail("nmf_eye_render: the plan was made for another frame size / field of view");
  const int n_ommatidia = plan->n_omm;
  const int16_t* const id_map_dev = plan->id_map; const void* const plan_dev = plan->rplan; const uint8_t* const pale_dev = plan->pale; const float* const inv_norm_dev = plan->inv_norm;
  if (!frames_out_dev && !omm_out_dev) return fail("nmf_eye_render: nothing to write");
  if (p->height <= 0 || p->width <= 0 || (p->height * p->width) % 16) return fail("nmf_eye_render: height * width must be a positive multiple of 16");
  if (n_ommatidia <= 0 || n_ommatidia > nmf::kMaxOmmatidia) return fail("nmf_eye_render: need 0 < n_ommatidia <= 1024");
  if (p->n_spheres < 0 || p->n_spheres > nmf::kMaxSpheres || (p->n_spheres > 0 && !spheres_dev)) return fail("nmf_eye_render: bad sphere list");
  if (p->n_capsules < 0 || p->n_capsules > nmf::kMaxCaps || (p->n_capsules > 0 && (!capsule_seg_dev || !capsule_geom_dev)))
    return fail("nmf_eye_render: bad body-capsule list (at most 64)");
  if (!(p->checker_size > 0.f) || !(p->fov_deg > 0.f) || p->fov_deg > 360.f) return fail("nmf_eye_render: bad checker size / field of view");
  const nmf_model* m = b->model;
  DEVICE_GUARD(b);
  if (b->dm.plane[0] != 0.f || b->dm.plane[1] != 0.f || b->dm.plane[2] != 1.f) return fail("nmf_eye_render: the ground plane must be z-up");
  if ((reinterpret_cast<uintptr_t>(plan_dev) | reinterpret_cast<uintptr_t>(frames_out_dev)) & 15u)
    return fail("nmf_eye_render: plan / frames must be 16-byte aligned");
  nmf::EyeArgs A{};
  A.height = p->height; A.width = p->width;
  A.half_fov = 0.5f * p->fov_deg * 3.14159265358979323846f / 180.f;
  for (int e = 0; e < 2; ++e) {
    if (p->eye_seg[e] < 0 || p->eye_seg[e] >= m->nseg) return fail("nmf_eye_render: eye segment out of range");
    A.eye_seg[e] = p->eye_seg[e];
    for (int i = 0; i < 3; ++i) A.rel_pos[e][i] = p->rel_pos[e][i];
    double w = p->rel_quat[e][0], x = p->rel_quat[e][1], y = p->rel_quat[e][2], z = p->rel_quat[e][3];
    const double n = std::sqrt(w * w + x * x + y * y + z * z);
    if (!(n > 0.0)) return fail("nmf_eye_render: zero camera quaternion");
    w /= n; x /= n; y /= n; z /= n;
    const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                         2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                         2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
    for (int i = 0; i < 9; ++i) A.rel_mat[e][i] = (float)R[i];
  }
  fill_scene(A, *p, b, 5);
  A.n_caps = p->n_capsules;
  for (int c = 0; c < 3; ++c) A.rgb[4][c] = p->body_rgb[c];
  if (p->rays_per_ommatidium != 0 && p->rays_per_ommatidium != nmf::kEyeRays) return fail("nmf_eye_render: rays_per_ommatidium must be 0 (every pixel) or 16");
  if (p->rays_per_ommatidium != 0 && frames_out_dev) return fail("nmf_eye_render: the sampled mode renders no frames (rays_per_ommatidium = 0 does)");
  A.sampled = p->rays_per_ommatidium;
  const int mode = A.sampled ? 2 : frames_out_dev ? 1 : 0;
#define NMF_EYE_LAUNCH(SAMPLED, RELIEF, FRAMES)                                                                                      \
  hipLaunchKernelGGL((nmf::nmf_eye_kernel<SAMPLED, RELIEF, FRAMES>), dim3((unsigned)(2 * b->n_worlds)), dim3(nmf::kEyeThreads), 0, (hipStream_t)stream, A, \
                     b->st.seg_xpos, b->st.seg_xquat, m->nseg, spheres_dev ? spheres_dev : b->st.seg_xpos,                           \
                     capsule_seg_dev, capsule_geom_dev, reinterpret_cast<const nmf::u32x4*>(plan_dev),                               \
                     plan->visit[mode], plan->cones[mode], reinterpret_cast<const float4*>(plan->chunk_cones[mode]), plan->n_groups[mode], \
                     id_map_dev, plan->slot_omm, pale_dev, inv_norm_dev, n_ommatidia, frames_out_dev, omm_out_dev)
  if (A.terrain_kind != 0) { if (A.sampled) NMF_EYE_LAUNCH(true, true, false); else if (frames_out_dev) NMF_EYE_LAUNCH(false, true, true); else NMF_EYE_LAUNCH(false, true, false); }
  else { if (A.sampled) NMF_EYE_LAUNCH(true, false, false); else if (frames_out_dev) NMF_EYE_LAUNCH(false, false, true); else NMF_EYE_LAUNCH(false, false, false); }
#undef NMF_EYE_LAUNCH
  HIP_OK(hipGetLastError());
  return 0;
}

// ---- batch camera renderer (nmf_camera.hip) ----
// Everything a render needs besides the batches' poses and the caller's spheres: an explicit handle with its own device copies.
// One plan type for both entries: nmf_camera_plan_create makes a plan of one fly that nmf_camera_render draws with
// nmf_camera_kernel, nmf_camera_plan_create_flies one of `flies.n_flies` flies for nmf_camera_render_flies.
struct nmf_camera_plan {
  const nmf_batch* batch = nullptr;           // the first fly's batch: the plan's device, and the owner nmf_camera_render asks for
  bool several = false;                       // made by nmf_camera_plan_create_flies
  int n_cameras = 0, n_selected = 0;
  nmf::CamArgs args{};
  nmf::CamFlies flies{};                      // per fly: the batch's pose arrays, the plan's copies of the capsule arrays
  nmf::CamView* views = nullptr; int* world_ids = nullptr;
  DevMem mem;
};

static_assert(NMF_CAMERA_MAX_FLIES == nmf::kCamMaxFlies && NMF_CAMERA_MAX == nmf::kCamMaxViews && NMF_CAMERA_MAX_CAPSULES == nmf::kCamMaxCaps,
              "include/nmf.h and nmf_camera.hip disagree on the renderer's limits");

extern "C" size_t nmf_camera_params_size(void) { return sizeof(nmf_camera_params); }

extern "C" void nmf_camera_plan_destroy(nmf_camera_plan* P) {
  if (!P) return;
  P->mem.release();
  delete P;
}

// `who`: the entry point, for the error texts.  cam_fly: null = every camera belongs to fly 0.
static int fill_camera_plan(nmf_camera_plan* P, const std::string& who, const nmf_camera_fly* flies, int n_flies, const nmf_camera_params* p,
                            const int32_t* cam_fly, int n_cameras, const int32_t* world_ids, int n_selected) {
  const nmf_batch* b = flies[0].batch;
  if (n_cameras < 1 || n_cameras > NMF_CAMERA_MAX) return fail(who + ": need 1 <= n_cameras <= 8");
  if (p->height < 1 || p->width < 1 || (int64_t)p->height * p->width > (1 << 26)) return fail(who + ": height and width must be at least 1 (and height * width at most 2^26)");
  if (!world_ids || n_selected < 1) return fail(who + ": at least one world must be selected");
  std::vector<char> seen((size_t)b->n_worlds, 0);
  for (int i = 0; i < n_selected; ++i) {
    if (world_ids[i] < 0 || world_ids[i] >= b->n_worlds) return fail(who + ": world id " + std::to_string(world_ids[i]) + " is outside [0, " + std::to_string(b->n_worlds) + ")");
    if (seen[(size_t)world_ids[i]]) return fail(who + ": world id " + std::to_string(world_ids[i]) + " is selected twice");
    seen[(size_t)world_ids[i]] = 1;
  }
  for (int f = 0; f < n_flies; ++f) {
    const nmf_camera_fly& F = flies[f];
    if (F.n_caps < 0 || F.n_caps > NMF_CAMERA_MAX_CAPSULES || (F.n_caps > 0 && (!F.cap_seg || !F.cap_geom || !F.cap_rgb))) return fail(who + ": bad capsule list (at most 72)");
    for (int c = 0; c < F.n_caps; ++c) {
      if (F.cap_seg[c] < 0 || F.cap_seg[c] >= F.batch->model->nseg) return fail(who + ": capsule segment out of range");
      if (!(F.cap_geom[7 * c + 6] > 0.f)) return fail(who + ": a capsule needs a positive radius");
    }
  }
  if (p->n_spheres < 0 || p->n_spheres > nmf::kMaxSpheres) return fail(who + ": at most 8 spheres");
  if (!(p->checker_size > 0.f)) return fail(who + ": bad checker size");
  if (!(p->ambient >= 0.f) || !(p->diffuse >= 0.f)) return fail(who + ": the light terms must not be negative");
  if (b->dm.plane[0] != 0.f || b->dm.plane[1] != 0.f || b->dm.plane[2] != 1.f) return fail(who + ": the ground plane must be z-up");
  std::vector<nmf::CamView> views((size_t)n_cameras);
  for (int c = 0; c < n_cameras; ++c) {
    const nmf_camera_view& v = p->cam[c];
    const int owner = cam_fly ? cam_fly[c] : 0;
    if (owner < 0 || owner >= n_flies) return fail(who + ": cam_fly[" + std::to_string(c) + "] = " + std::to_string(owner) + " is outside [0, n_flies)");
    if (v.mode != NMF_CAMERA_FIXED && v.mode != NMF_CAMERA_TRACK) return fail(who + ": camera mode must be NMF_CAMERA_FIXED or NMF_CAMERA_TRACK");
    if (v.mode == NMF_CAMERA_TRACK && (v.track_seg < 0 || v.track_seg >= flies[owner].batch->model->nseg)) return fail(who + ": tracked segment out of range");
    if (!(v.fovy_deg > 0.f) || !(v.fovy_deg < 180.f)) return fail(who + ": need 0 < fovy < 180 degrees");
    for (int i = 0; i < 3; ++i)          // orthonormal columns
      for (int j = i; j < 3; ++j) {
        const double dd = (double)v.rot[i] * v.rot[j] + (double)v.rot[3 + i] * v.rot[3 + j] + (double)v.rot[6 + i] * v.rot[6 + j];
        if (!(std::fabs(dd - (i == j ? 1.0 : 0.0)) < 1e-4)) return fail(who + ": the camera rotation must be orthonormal");
      }
    views[c].mode = v.mode; views[c].seg = v.mode == NMF_CAMERA_TRACK ? v.track_seg : 0;
    for (int i = 0; i < 3; ++i) views[c].pos[i] = v.pos[i];
    for (int i = 0; i < 9; ++i) views[c].rot[i] = v.rot[i];
    views[c].tan_px = (float)(std::tan(0.5 * (double)v.fovy_deg * 3.14159265358979323846 / 180.0) / (0.5 * (double)p->height));
    P->flies.cam_fly[c] = owner;
  }
  nmf::CamArgs& A = P->args;
  A.height = p->height; A.width = p->width; A.tiles_x = (p->width + nmf::kCamTile - 1) / nmf::kCamTile;
  A.ambient = p->ambient; A.diffuse = p->diffuse;
  fill_scene(A, *p, b, 4);
  A.n_caps = flies[0].n_caps;
  P->n_cameras = n_cameras; P->n_selected = n_selected;
  P->views = (nmf::CamView*)P->mem.upload(views.data(), sizeof(nmf::CamView) * views.size());
  P->world_ids = (int*)P->mem.upload(world_ids, sizeof(int) * (size_t)n_selected);
  P->flies.n_flies = n_flies;
  for (int f = 0; f < n_flies; ++f) {
    const nmf_camera_fly& F = flies[f];
    const int n_caps = F.n_caps;
    std::vector<unsigned int> rgbw((size_t)std::max(n_caps, 1), 0u);
    for (int c = 0; c < n_caps; ++c) rgbw[(size_t)c] = (unsigned int)F.cap_rgb[3 * c] | ((unsigned int)F.cap_rgb[3 * c + 1] << 8) | ((unsigned int)F.cap_rgb[3 * c + 2] << 16);
    nmf::CamFly& D = P->flies.fly[f];
    D.seg_xpos = F.batch->st.seg_xpos; D.seg_xquat = F.batch->st.seg_xquat; D.nseg = F.batch->model->nseg; D.n_caps = n_caps;
    D.cap_seg = (const int*)P->mem.upload(F.cap_seg, sizeof(int) * (size_t)n_caps);
    D.cap_geom = (const float*)P->mem.upload(F.cap_geom, sizeof(float) * 7 * (size_t)n_caps);
    D.cap_rgb = (const unsigned int*)P->mem.upload(rgbw.data(), sizeof(unsigned int) * (size_t)n_caps);
  }
  if (!P->mem.ok) return -1;
  HIP_OK(hipDeviceSynchronize());
  return 0;
}

extern "C" nmf_camera_plan* nmf_camera_plan_create(nmf_batch* b, const nmf_camera_params* p, int n_cameras, const int32_t* world_ids, int n_selected,
                                                   const int32_t* cap_seg, const float* cap_geom, const uint8_t* cap_rgb, int n_caps) {
  if (!b || !p) { fail("nmf_camera_plan_create: null batch / params"); return nullptr; }
  return build_or_destroy(b->mem.device, "nmf_camera_plan_create", new nmf_camera_plan(), nmf_camera_plan_destroy, [&](nmf_camera_plan* P) {
    P->batch = b;
    const nmf_camera_fly one{b, cap_seg, cap_geom, cap_rgb, n_caps};
    return fill_camera_plan(P, "nmf_camera_plan_create", &one, 1, p, nullptr, n_cameras, world_ids, n_selected);
  });
}

extern "C" nmf_camera_plan* nmf_camera_plan_create_flies(const nmf_camera_fly* flies, int n_flies, const nmf_camera_params* p, const int32_t* cam_fly,
                                                         int n_cameras, const int32_t* world_ids, int n_selected) {
  const std::string who = "nmf_camera_plan_create_flies";
  if (!flies || !p || !cam_fly) { fail(who + ": null flies / params / cam_fly"); return nullptr; }
  if (n_flies < 1 || n_flies > NMF_CAMERA_MAX_FLIES) { fail(who + ": need 1 <= n_flies <= NMF_CAMERA_MAX_FLIES = " + std::to_string(NMF_CAMERA_MAX_FLIES) + ", got " + std::to_string(n_flies)); return nullptr; }
  for (int f = 0; f < n_flies; ++f)
    if (!flies[f].batch) { fail(who + ": the batch of fly " + std::to_string(f) + " is null"); return nullptr; }
  const nmf_batch* b = flies[0].batch;
  for (int f = 1; f < n_flies; ++f) {
    const nmf_batch* o = flies[f].batch;
    const std::string fly = who + ": the batch of fly " + std::to_string(f);
    if (o->mem.device != b->mem.device) { fail(fly + " is on another device than fly 0's"); return nullptr; }
    if (o->n_worlds != b->n_worlds) { fail(fly + " has " + std::to_string(o->n_worlds) + " worlds, fly 0's has " + std::to_string(b->n_worlds)); return nullptr; }
    if (std::memcmp(o->dm.plane, b->dm.plane, sizeof(b->dm.plane)) != 0) { fail(fly + " has another ground plane than fly 0's"); return nullptr; }
    if (o->dm.terrain_type != b->dm.terrain_type || std::memcmp(o->dm.terrain, b->dm.terrain, sizeof(b->dm.terrain)) != 0) { fail(fly + " has another terrain than fly 0's"); return nullptr; }
  }
  return build_or_destroy(b->mem.device, "nmf_camera_plan_create_flies", new nmf_camera_plan(), nmf_camera_plan_destroy, [&](nmf_camera_plan* P) {
    P->batch = b; P->several = true;
    return fill_camera_plan(P, who, flies, n_flies, p, cam_fly, n_cameras, world_ids, n_selected);
  });
}

static int camera_render_args(const std::string& who, const nmf_camera_plan* P, const float* spheres_dev, const uint8_t* frames_out_dev) {
  if (!frames_out_dev) return fail(who + ": nothing to write");
  if (reinterpret_cast<uintptr_t>(frames_out_dev) & 15u) return fail(who + ": frames must be 16-byte aligned");
  if (P->args.n_spheres > 0 && !spheres_dev) return fail(who + ": the plan has spheres, spheres_dev is required");
  return 0;
}

// Pure stream-ordered work: argument checks on the host, one kernel launch.
extern "C" int nmf_camera_render(nmf_batch* b, const nmf_camera_plan* P, const float* spheres_dev, uint8_t* frames_out_dev, void* stream) {
  if (!b || !P) return fail("nmf_camera_render: null batch / plan");
  if (P->several) return fail("nmf_camera_render: the plan has several flies: nmf_camera_render_flies");
  if (P->batch != b) return fail("nmf_camera_render: the plan was made for another batch");
  if (camera_render_args("nmf_camera_render", P, spheres_dev, frames_out_dev) != 0) return -1;
  DEVICE_GUARD(b);
  const nmf::CamArgs& A = P->args;
  const nmf::CamFly& F = P->flies.fly[0];
  const unsigned tiles = (unsigned)(A.tiles_x * ((A.height + nmf::kCamTile - 1) / nmf::kCamTile));
  hipLaunchKernelGGL(nmf::nmf_camera_kernel, dim3(tiles, (unsigned)P->n_cameras, (unsigned)P->n_selected), dim3(nmf::kCamThreads), 0, (hipStream_t)stream, A,
                     P->views, P->world_ids, F.seg_xpos, F.seg_xquat, F.nseg, spheres_dev ? spheres_dev : F.seg_xpos,
                     F.cap_seg, F.cap_geom, F.cap_rgb, frames_out_dev);
  HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int nmf_camera_render_flies(const nmf_camera_plan* P, const float* spheres_dev, uint8_t* frames_out_dev, void* stream) {
  if (!P) return fail("nmf_camera_render_flies: null plan");
  if (!P->several) return fail("nmf_camera_render_flies: the plan has one fly's batch: nmf_camera_render");
  if (camera_render_args("nmf_camera_render_flies", P, spheres_dev, frames_out_dev) != 0) return -1;
  DEVICE_GUARD(P->batch);
  const nmf::CamArgs& A = P->args;
  const unsigned tiles = (unsigned)(A.tiles_x * ((A.height + nmf::kCamTile - 1) / nmf::kCamTile));
  hipLaunchKernelGGL(nmf::nmf_camera_flies_kernel, dim3(tiles, (unsigned)P->n_cameras, (unsigned)P->n_selected), dim3(nmf::kCamThreads), 0, (hipStream_t)stream, A,
                     P->flies, P->views, P->world_ids, spheres_dev ? spheres_dev : P->flies.fly[0].seg_xpos, frames_out_dev);
  HIP_OK(hipGetLastError());
  return 0;
}

// The entry without a plan handle: plans are built on first use and kept per batch (up to four, least recently used first out), keyed
// on the ADDRESSES of the four buffers + shape + lens.  The first call with a new key is therefore NOT stream-ordered (see
// nmf_eye_plan_create) and must not sit inside a stream capture, and a caller that rewrites a buffer in place must make a new
// plan (nmf_eye_plan_create) — include/nmf.h says so at the declaration.
extern "C" int nmf_eye_render(nmf_batch* b, const nmf_eye_params* p, const float* spheres_dev, const int32_t* capsule_seg_dev,
                              const float* capsule_geom_dev, const int16_t* id_map_dev,
                              const void* plan_dev, const uint8_t* pale_dev, const float* inv_norm_dev, int n_ommatidia,
                              uint8_t* frames_out_dev, float* omm_out_dev, void* stream) {
  if (!b || !p) return fail("nmf_eye_render: null batch / params");
  if (!id_map_dev || !plan_dev || !pale_dev || !inv_norm_dev) return fail("nmf_eye_render: id map, plan, pale and inv_norm are required");
  auto& L = b->eye_plans;
  nmf_eye_plan* plan = nullptr;
  for (size_t i = 0; i < L.size(); ++i) {
    nmf_eye_plan* q = L[i];
    if (q->key[0] == id_map_dev && q->key[1] == plan_dev && q->key[2] == pale_dev && q->key[3] == inv_norm_dev && q->h == p->height && q->w == p->width &&
        q->fov == p->fov_deg && q->n_omm == n_ommatidia) { plan = q; L.erase(L.begin() + (long)i); L.push_back(q); break; }
  }
  if (!plan) {
    plan = nmf_eye_plan_create(id_map_dev, plan_dev, pale_dev, inv_norm_dev, p->height, p->width, p->fov_deg, n_ommatidia, b->mem.device);
    if (!plan) return -1;
    plan->key[0] = id_map_dev; plan->key[1] = plan_dev; plan->key[2] = pale_dev; plan->key[3] = inv_norm_dev;
    if (L.size() >= 4) { nmf_eye_plan_destroy(L.front()); L.erase(L.begin()); }
    L.push_back(plan);
  }
  return nmf_eye_render_planned(b, p, plan, spheres_dev, capsule_seg_dev, capsule_geom_dev, frames_out_dev, omm_out_dev, stream);
}

// ---- closed-loop tripod CPG (nmf_cpg.hip) ----
// The controller's shared tables (own device copies) and its per-world state.
struct nmf_cpg {
  int n_worlds = 0, table_steps = 0;
  nmf::CpgArgs args{};
  float* cycle = nullptr; float* mean = nullptr; int* leg_of_col = nullptr; uint8_t* stance = nullptr;
  double* phase = nullptr; float* mag = nullptr; double* mag_acc = nullptr; float* drive = nullptr;   // mag_acc: the magnitudes' float64 sums
  // the hybrid rules (nmf_cpg_hybrid_enable): the batch whose pose / sensor outputs the decision reads, and the rules' state
  const nmf_batch* batch = nullptr;
  bool hybrid = false;
  nmf::CpgHybridArgs hargs{};
  nmf::CpgHybridPtrs hptrs{};
  DevMem mem;
};

extern "C" size_t nmf_cpg_params_size(void) { return sizeof(nmf_cpg_params); }

extern "C" void nmf_cpg_destroy(nmf_cpg* C) {
  if (!C) return;
  C->mem.release();
  delete C;
}

extern "C" int nmf_cpg_reset(nmf_cpg* C, const uint8_t* mask_dev, int first_world, int total_worlds, void* stream) {
  if (!C) return fail("nmf_cpg_reset: null controller");
  if (first_world < 0 || total_worlds < 1 || (int64_t)first_world + C->n_worlds > (int64_t)total_worlds)
    return fail("nmf_cpg_reset: the controller's worlds [first_world, first_world + n_worlds) must lie inside [0, total_worlds)");
  DEVICE_GUARD(C);
  const dim3 grid((unsigned)((6 * C->n_worlds + 255) / 256)), block(256);
  hipLaunchKernelGGL(nmf::nmf_cpg_reset_kernel, grid, block, 0, (hipStream_t)stream,
                     C->n_worlds, mask_dev, first_world, total_worlds, C->phase, C->mag, C->mag_acc, C->drive);
  HIP_OK(hipGetLastError());
  if (C->hybrid) {
    hipLaunchKernelGGL(nmf::nmf_cpg_hybrid_reset_kernel, grid, block, 0, (hipStream_t)stream,
                       C->n_worlds, mask_dev, C->hptrs.retraction, C->hptrs.stumbling, C->hptrs.flags);
    HIP_OK(hipGetLastError());
  }
  return 0;
}

static int fill_cpg(nmf_cpg* C, const nmf_cpg_params* p, const float* cycle, const int32_t* leg_of_col, const uint8_t* stance) {
  if (p->n_pos < 1 || p->n_pos > 4096) return fail("nmf_cpg_create: need 1 <= n_pos <= 4096 position columns");
  if (p->n_bins < 2 || p->n_bins > (1 << 20)) return fail("nmf_cpg_create: need 2 <= n_bins <= 2^20 phase bins");
  if (p->table_steps < 1) return fail("nmf_cpg_create: table_steps must be at least 1");
  if (!(p->timestep > 0.0) || !std::isfinite(p->frequency) || !std::isfinite(p->coupling) || !std::isfinite(p->convergence))
    return fail("nmf_cpg_create: the timestep must be positive, frequency / coupling / convergence finite");
  if (!cycle || !leg_of_col) return fail("nmf_cpg_create: cycle and leg_of_col are required");
  for (int c = 0; c < p->n_pos; ++c)
    if (leg_of_col[c] < 0 || leg_of_col[c] > 5) return fail("nmf_cpg_create: leg_of_col[" + std::to_string(c) + "] is outside 0..5");
  nmf::CpgArgs& A = C->args;
  A.n_worlds = C->n_worlds; A.n_pos = p->n_pos; A.n_act = p->n_pos + (stance ? 6 : 0); A.n_bins = p->n_bins;
  A.frequency = p->frequency; A.timestep = p->timestep;
  A.coupling = p->coupling; A.convergence = p->convergence; A.adhesion_on = p->adhesion_on; A.adhesion_off = p->adhesion_off;
  C->table_steps = p->table_steps;
  std::vector<float> mean((size_t)p->n_pos);
  for (int c = 0; c < p->n_pos; ++c) {
    double sum = 0.0;
    for (int i = 0; i < p->n_bins; ++i) sum += (double)cycle[(size_t)i * p->n_pos + c];
    mean[(size_t)c] = (float)(sum / (double)p->n_bins);
  }
  const size_t n = (size_t)C->n_worlds;
  C->cycle = (float*)C->mem.upload(cycle, sizeof(float) * (size_t)p->n_bins * (size_t)p->n_pos);
  C->mean = (float*)C->mem.upload(mean.data(), sizeof(float) * mean.size());
  C->leg_of_col = (int*)C->mem.upload(leg_of_col, sizeof(int) * (size_t)p->n_pos);
  C->stance = (uint8_t*)C->mem.upload(stance, stance ? (size_t)p->n_bins * 6 : 0);
  C->phase = (double*)C->mem.alloc(sizeof(double) * 6 * n);
  C->mag = (float*)C->mem.alloc(sizeof(float) * 6 * n);
  C->mag_acc = (double*)C->mem.alloc(sizeof(double) * 6 * n);
  C->drive = (float*)C->mem.alloc(sizeof(float) * 2 * n);
  if (!C->mem.ok) return -1;
  if (nmf_cpg_reset(C, nullptr, 0, C->n_worlds, nullptr) != 0) return -1;
  HIP_OK(hipDeviceSynchronize());
  return 0;
}

extern "C" nmf_cpg* nmf_cpg_create(nmf_batch* b, const nmf_cpg_params* p, const float* cycle, const int32_t* leg_of_col, const uint8_t* stance) {
  if (!b || !p) { fail("nmf_cpg_create: null batch / params"); return nullptr; }
  return build_or_destroy(b->mem.device, "nmf_cpg_create", new nmf_cpg(), nmf_cpg_destroy, [&](nmf_cpg* C) {
    C->n_worlds = b->n_worlds; C->batch = b;
    return fill_cpg(C, p, cycle, leg_of_col, stance);
  });
}

extern "C" void* nmf_cpg_field_ptr(nmf_cpg* C, int which, int32_t* width) {
  if (!C) { fail("nmf_cpg_field_ptr: null controller"); return nullptr; }
  void* ptr[6] = {C->phase, C->mag, C->drive, C->hptrs.retraction, C->hptrs.stumbling, C->hptrs.flags};
  const int32_t w[6] = {6, 6, 2, 6, 6, 6};
  if (which < 0 || which > 5) { fail("nmf_cpg_field_ptr: no such field"); return nullptr; }
  if (which > 2 && !C->hybrid) { fail("nmf_cpg_field_ptr: the hybrid rules are not enabled (nmf_cpg_hybrid_enable)"); return nullptr; }
  if (width) *width = w[which];
  return ptr[which];
}

// What every advance of a controller (nmf_cpg_advance, nmf_cpg_advance_hybrid, nmf_rules_advance) checks of its table before it
// launches; `made_for`: the controller's table_steps, `device`: its device, which the caller has made current.
static int check_table(const std::string& w, int made_for, int device, int n_steps, float* table_dev, int table_steps, void* stream) {
  if (!table_dev) return fail(w + ": null table");
  if (table_steps != made_for) return fail(w + ": the controller was made for tables of " + std::to_string(made_for) + " steps, got " + std::to_string(table_steps));
  if (n_steps < 1 || n_steps > table_steps) return fail(w + ": n_steps must be in 1.." + std::to_string(table_steps) + ", got " + std::to_string(n_steps));
  // the table must live on the controller's device (a pointer query is no stream work, but a capture is left alone)
  hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing((hipStream_t)stream, &capturing) == hipSuccess && capturing == hipStreamCaptureStatusNone) {
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, table_dev) != hipSuccess) { (void)hipGetLastError(); return fail(w + ": the table is not device memory"); }
    if (at.device != device) return fail(w + ": the controller was made for device " + std::to_string(device) + ", the table is on device " + std::to_string(at.device));
  }
  return 0;
}

// Pure stream-ordered work: argument checks on the host, one kernel launch (with the hybrid rules or without).
static int cpg_advance(const char* who, bool hybrid, nmf_cpg* C, int n_steps, float* table_dev, int table_steps, void* stream) {
  const std::string w(who);
  if (!C) return fail(w + ": null controller");
  DEVICE_GUARD(C);
  if (check_table(w, C->table_steps, C->mem.device, n_steps, table_dev, table_steps, stream) != 0) return -1;
  if (hybrid && !C->hybrid) return fail(w + ": the hybrid rules are not enabled (nmf_cpg_hybrid_enable)");
  const dim3 grid((unsigned)((C->n_worlds + nmf::kCpgWorlds - 1) / nmf::kCpgWorlds)), block(nmf::kCpgThreads);
  if (hybrid)
    hipLaunchKernelGGL(nmf::nmf_cpg_advance_hybrid_kernel, grid, block, 0, (hipStream_t)stream, C->args, C->hargs, C->hptrs, C->cycle, C->mean,
                       C->leg_of_col, C->stance, C->drive, C->phase, C->mag, C->mag_acc, table_dev, table_steps, n_steps);
  else
    hipLaunchKernelGGL(nmf::nmf_cpg_advance_kernel, grid, block, 0, (hipStream_t)stream, C->args, C->cycle, C->mean, C->leg_of_col, C->stance,
                       C->drive, C->phase, C->mag, C->mag_acc, table_dev, table_steps, n_steps);
  HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int nmf_cpg_advance(nmf_cpg* C, int n_steps, float* table_dev, int table_steps, void* stream) {
  return cpg_advance("nmf_cpg_advance", false, C, n_steps, table_dev, table_steps, stream);
}

// ---- the hybrid rules of the CPG (retraction, stumbling) ----
extern "C" size_t nmf_cpg_hybrid_params_size(void) { return sizeof(nmf_cpg_hybrid_params); }

extern "C" int nmf_cpg_hybrid_enable(nmf_cpg* C, const nmf_cpg_hybrid_params* p, const float* corr, const uint8_t* swing, int root_seg,
                                     const int32_t tip_seg[6]) {
  if (!C) return fail("nmf_cpg_hybrid_enable: null controller");
  if (!p || !corr || !swing || !tip_seg) return fail("nmf_cpg_hybrid_enable: params, corr, swing and tip_seg are required");
  if (C->hybrid) return fail("nmf_cpg_hybrid_enable: the hybrid rules of this controller are already enabled");
  const nmf_batch* b = C->batch;
  if (b->model->nsensor == 0 || !b->st.sensordata) return fail("nmf_cpg_hybrid_enable: the batch's model has no leg sensors (nsensor == 0)");
  if (b->widths[NMF_SENSORDATA] != 96)
    return fail("nmf_cpg_hybrid_enable: the batch's sensordata is " + std::to_string(b->widths[NMF_SENSORDATA]) + " wide, the rules read six leg sensors of 16 values");
  const int nseg = b->model->nseg;
  if (root_seg < 0 || root_seg >= nseg) return fail("nmf_cpg_hybrid_enable: root_seg " + std::to_string(root_seg) + " is outside the batch's " + std::to_string(nseg) + " segments");
  for (int l = 0; l < 6; ++l)
    if (tip_seg[l] < 0 || tip_seg[l] >= nseg) return fail("nmf_cpg_hybrid_enable: tip_seg[" + std::to_string(l) + "] = " + std::to_string(tip_seg[l]) + " is outside the batch's " + std::to_string(nseg) + " segments");
  const float checked[7] = {p->retraction_threshold, p->stumbling_force_threshold, p->retraction_up, p->retraction_down, p->stumbling_up, p->stumbling_down, p->max_correction};
  for (float v : checked)
    if (!(v >= 0.f) || !std::isfinite(v)) return fail("nmf_cpg_hybrid_enable: thresholds, rates and max_correction must be finite and not negative");
  for (int c = 0; c < C->args.n_pos; ++c)
    if (!std::isfinite(corr[c])) return fail("nmf_cpg_hybrid_enable: corr[" + std::to_string(c) + "] is not finite");
  DEVICE_GUARD(C);
  nmf::CpgHybridArgs H{};
  H.nseg = nseg; H.root_seg = root_seg; H.contact_frame = b->dm.sem_sensor_contact_frame;
  for (int l = 0; l < 6; ++l) H.tip_seg[l] = tip_seg[l];
  H.retraction_threshold = p->retraction_threshold; H.stumbling_force_threshold = p->stumbling_force_threshold;
  H.up_r = (float)(C->args.timestep * (double)p->retraction_up); H.down_r = (float)(C->args.timestep * (double)p->retraction_down);
  H.up_s = (float)(C->args.timestep * (double)p->stumbling_up); H.down_s = (float)(C->args.timestep * (double)p->stumbling_down);
  H.cap = p->max_correction;
  const size_t n = (size_t)C->n_worlds, mark = C->mem.mark();
  C->mem.who = "nmf_cpg_hybrid_enable";
  nmf::CpgHybridPtrs P{};
  P.corr = (const float*)C->mem.upload(corr, sizeof(float) * (size_t)C->args.n_pos);
  P.swing = (const uint8_t*)C->mem.upload(swing, (size_t)C->args.n_bins * 6);
  P.retraction = (float*)C->mem.alloc(sizeof(float) * 6 * n);
  P.stumbling = (float*)C->mem.alloc(sizeof(float) * 6 * n);
  P.flags = (uint8_t*)C->mem.alloc(6 * n);
  P.seg_xpos = b->st.seg_xpos; P.seg_xquat = b->st.seg_xquat; P.sensordata = b->st.sensordata;
  if (!C->mem.ok) {
    (void)hipGetLastError();
    C->mem.rollback(mark);        // the controller stays as it was
    return -1;
  }
  HIP_OK(hipDeviceSynchronize());
  C->hargs = H;
  C->hptrs = P;
  C->hybrid = true;
  return 0;
}

extern "C" int nmf_cpg_advance_hybrid(nmf_cpg* C, int n_steps, float* table_dev, int table_steps, void* stream) {
  return cpg_advance("nmf_cpg_advance_hybrid", true, C, n_steps, table_dev, table_steps, stream);
}

// ---- advected odor plumes (nmf_plume.hip) ----
// The shared maps (own device copies) and the per-plume state; the batch lends its pose arrays to nmf_plume_sample_sites.
struct nmf_plume {
  const nmf_batch* batch = nullptr;
  int n_worlds = 0;
  nmf::PlumeArgs args{};
  float* source = nullptr; float* eddies = nullptr;
  float* grid[2] = {nullptr, nullptr}; float* wind = nullptr; unsigned int* ticks = nullptr; int* parity = nullptr;
  DevMem mem;
};

extern "C" size_t nmf_plume_params_size(void) { return sizeof(nmf_plume_params); }

extern "C" void nmf_plume_destroy(nmf_plume* P) {
  if (!P) return;
  P->mem.release();
  delete P;
}

extern "C" int nmf_plume_reset(nmf_plume* P, const uint8_t* mask_dev, void* stream) {
  if (!P) return fail("nmf_plume_reset: null plume");
  DEVICE_GUARD(P);
  const size_t total = (size_t)P->args.n_plumes * (size_t)P->args.H * (size_t)P->args.W;
  hipLaunchKernelGGL(nmf::nmf_plume_reset_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     P->args, mask_dev, P->grid[0], P->grid[1], P->wind, P->ticks);
  HIP_OK(hipGetLastError());
  return 0;
}

static int fill_plume(nmf_plume* P, const nmf_plume_params* p, const float* source, const float* eddies) {
  if (p->n_plumes != 1 && p->n_plumes != P->n_worlds)
    return fail("nmf_plume_create: n_plumes must be 1 or the batch's n_worlds (" + std::to_string(P->n_worlds) + "), got " + std::to_string(p->n_plumes));
  if (p->height < 8 || p->height > 1024 || p->width < 8 || p->width > 1024)
    return fail("nmf_plume_create: need 8 <= height, width <= 1024 cells, got " + std::to_string(p->height) + " x " + std::to_string(p->width));
  if (p->first_world < 0) return fail("nmf_plume_create: first_world must not be negative");
  const float values[11] = {p->cell_size, p->origin_x, p->origin_y, p->tick_s, p->diffusivity, p->mean_wind_x, p->mean_wind_y, p->wind_tau,
                            p->wind_sigma, p->eddy_gain, p->intensity_scale};
  for (float v : values)
    if (!std::isfinite(v)) return fail("nmf_plume_create: a parameter is not finite");
  if (!(p->cell_size > 0.f) || !(p->tick_s > 0.f) || !(p->wind_tau > 0.f))
    return fail("nmf_plume_create: cell_size, tick_s and wind_tau must be positive");
  if (p->diffusivity < 0.f || p->wind_sigma < 0.f) return fail("nmf_plume_create: diffusivity and wind_sigma must not be negative");
  const double h = p->cell_size, dt = p->tick_s, D = (double)p->diffusivity * dt / (h * h);
  if (D > 0.25) return fail("nmf_plume_create: diffusivity tick_s / cell_size^2 = " + std::to_string(D) + " exceeds 1/4 (the explicit diffusion step is unstable)");
  if (!source) return fail("nmf_plume_create: the source map is required");
  const size_t cells = (size_t)p->height * (size_t)p->width, n = (size_t)p->n_plumes;
  for (size_t c = 0; c < cells; ++c)
    if (!std::isfinite(source[c])) return fail("nmf_plume_create: source[" + std::to_string(c) + "] is not finite");
  for (size_t c = 0; eddies && c < 2 * cells; ++c)
    if (!std::isfinite(eddies[c])) return fail("nmf_plume_create: eddies[" + std::to_string(c) + "] is not finite");
  nmf::PlumeArgs& A = P->args;
  A.n_plumes = p->n_plumes; A.H = p->height; A.W = p->width; A.first_world = p->first_world;
  A.x0 = p->origin_x; A.y0 = p->origin_y; A.h = p->cell_size; A.scale = p->intensity_scale;
  A.r = (float)(dt / h); A.D = (float)D; A.eddy_gain = p->eddy_gain;
  A.a = (float)(dt / (double)p->wind_tau); A.b = (float)((double)p->wind_sigma * std::sqrt(dt));
  A.mean_x = p->mean_wind_x; A.mean_y = p->mean_wind_y; A.seed = p->seed;
  P->source = (float*)P->mem.upload(source, sizeof(float) * cells);
  if (eddies) P->eddies = (float*)P->mem.upload(eddies, sizeof(float) * 2 * cells);
  for (float*& g : P->grid) g = (float*)P->mem.alloc(sizeof(float) * n * cells);
  P->wind = (float*)P->mem.alloc(sizeof(float) * 2 * n);
  P->ticks = (unsigned int*)P->mem.alloc(sizeof(unsigned int) * n);
  P->parity = (int*)P->mem.alloc(sizeof(int));
  if (!P->mem.ok) return -1;
  if (nmf_plume_reset(P, nullptr, nullptr) != 0) return -1;
  HIP_OK(hipDeviceSynchronize());
  return 0;
}

extern "C" nmf_plume* nmf_plume_create(nmf_batch* b, const nmf_plume_params* p, const float* source, const float* eddies) {
  if (!b || !p) { fail("nmf_plume_create: null batch / params"); return nullptr; }
  return build_or_destroy(b->mem.device, "nmf_plume_create", new nmf_plume(), nmf_plume_destroy, [&](nmf_plume* P) {
    P->n_worlds = b->n_worlds; P->batch = b;
    return fill_plume(P, p, source, eddies);
  });
}

extern "C" void* nmf_plume_field_ptr(nmf_plume* P, int which, int32_t* width) {
  if (!P) { fail("nmf_plume_field_ptr: null plume"); return nullptr; }
  void* ptr[5] = {P->wind, P->ticks, P->grid[0], P->grid[1], P->parity};
  const int32_t w[5] = {2, 1, P->args.H * P->args.W, P->args.H * P->args.W, 1};
  if (which < 0 || which > 4) { fail("nmf_plume_field_ptr: no such field"); return nullptr; }
  if (width) *width = w[which];
  return ptr[which];
}

// Pure stream-ordered work: per tick the grids from the old ones, then winds, tick counters and the parity word.
extern "C" int nmf_plume_advance(nmf_plume* P, int n_ticks, void* stream) {
  if (!P) return fail("nmf_plume_advance: null plume");
  if (n_ticks < 1) return fail("nmf_plume_advance: n_ticks must be at least 1, got " + std::to_string(n_ticks));
  DEVICE_GUARD(P);
  const nmf::PlumeArgs& A = P->args;
  const unsigned tiles = (unsigned)(((A.W + nmf::kPlumeTileW - 1) / nmf::kPlumeTileW) * ((A.H + nmf::kPlumeTileH - 1) / nmf::kPlumeTileH));
  for (int t = 0; t < n_ticks; ++t) {
    hipLaunchKernelGGL(nmf::nmf_plume_tick_kernel, dim3(tiles * (unsigned)A.n_plumes), dim3(nmf::kPlumeThreads), 0, (hipStream_t)stream,
                       A, P->parity, P->wind, P->eddies, P->source, P->grid[0], P->grid[1]);
    hipLaunchKernelGGL(nmf::nmf_plume_wind_kernel, dim3((unsigned)((A.n_plumes + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       A, P->parity, P->wind, P->ticks);
  }
  HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int nmf_plume_sample_points(nmf_plume* P, const float* points_dev, int n_pts, float* out_dev, uint8_t* oob_dev, void* stream) {
  if (!P) return fail("nmf_plume_sample_points: null plume");
  if (!points_dev || !out_dev || !oob_dev) return fail("nmf_plume_sample_points: null buffer");
  if (n_pts < 1) return fail("nmf_plume_sample_points: n_pts must be at least 1, got " + std::to_string(n_pts));
  DEVICE_GUARD(P);
  constexpr int per_block = nmf::kPlumeSampleThreads / nmf::kWave;
  hipLaunchKernelGGL(nmf::nmf_plume_sample_points_kernel, dim3((unsigned)((P->n_worlds + per_block - 1) / per_block)), dim3(nmf::kPlumeSampleThreads),
                     0, (hipStream_t)stream, P->args, P->n_worlds, P->parity, P->grid[0], P->grid[1], points_dev, n_pts, out_dev, oob_dev);
  HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int nmf_plume_sample_sites(nmf_plume* P, const int32_t* sensor_seg_dev, const float* sensor_rel_dev, int n_sensors, float* out_dev,
                                      uint8_t* oob_dev, void* stream) {
  if (!P) return fail("nmf_plume_sample_sites: null plume");
  if (!sensor_seg_dev || !sensor_rel_dev || !out_dev || !oob_dev) return fail("nmf_plume_sample_sites: null buffer");
  if (n_sensors < 1) return fail("nmf_plume_sample_sites: n_sensors must be at least 1, got " + std::to_string(n_sensors));
  DEVICE_GUARD(P);
  const nmf_batch* b = P->batch;
  constexpr int per_block = nmf::kPlumeSampleThreads / nmf::kWave;
  hipLaunchKernelGGL(nmf::nmf_plume_sample_sites_kernel, dim3((unsigned)((P->n_worlds + per_block - 1) / per_block)), dim3(nmf::kPlumeSampleThreads),
                     0, (hipStream_t)stream, P->args, P->n_worlds, P->parity, P->grid[0], P->grid[1], b->st.seg_xpos, b->st.seg_xquat,
                     b->model->nseg, sensor_seg_dev, sensor_rel_dev, n_sensors, out_dev, oob_dev);
  HIP_OK(hipGetLastError());
  return 0;
}

// ---- sensory steering (nmf_taxis.hip) ----
extern "C" size_t nmf_taxis_params_size(void) { return sizeof(nmf_taxis_params); }

extern "C" int nmf_taxis_update(const nmf_taxis_params* p, const int16_t* centres_dev, int n_omm, int height, int width, const float* omm_dev,
                                const float* odor_dev, const float* odor_gains_dev, int n_dims, int n_worlds, float* features_dev,
                                float* bias_dev, float* drive_dev, void* stream) {
  if (!p) return fail("nmf_taxis_update: null params");
  if (!drive_dev) return fail("nmf_taxis_update: null drive");
  if (!omm_dev && !odor_dev) return fail("nmf_taxis_update: omm and odor are both null (nothing to steer by)");
  if (n_worlds < 1) return fail("nmf_taxis_update: n_worlds must be at least 1, got " + std::to_string(n_worlds));
  if (n_dims < 0 || n_dims > nmf::kTaxisMaxDims) return fail("nmf_taxis_update: n_dims must be in 0..8, got " + std::to_string(n_dims));
  if (omm_dev) {
    if (n_omm < 1 || n_omm > nmf::kMaxOmmatidia) return fail("nmf_taxis_update: n_omm must be in 1..1024, got " + std::to_string(n_omm));
    if (height < 1 || height > nmf::kTaxisMaxSide || width < 1 || width > nmf::kTaxisMaxSide)
      return fail("nmf_taxis_update: need 1 <= height, width <= 2047 pixels, got " + std::to_string(height) + " x " + std::to_string(width));
    if (!centres_dev) return fail("nmf_taxis_update: null centres");
    if (((uintptr_t)centres_dev & 3) || ((uintptr_t)omm_dev & 7)) return fail("nmf_taxis_update: centres must be 4-byte and omm 8-byte aligned");
  }
  if (odor_dev) {
    if (n_dims > 0 && !odor_gains_dev) return fail("nmf_taxis_update: null odor gains");
    if ((uintptr_t)odor_dev & 15) return fail("nmf_taxis_update: odor must be 16-byte aligned");
  }
  nmf::TaxisArgs A;
  A.p = *p;
  A.n_worlds = n_worlds; A.n_omm = n_omm; A.n_dims = n_dims; A.H = height; A.W = width;
  constexpr int per_block = nmf::kTaxisThreads / nmf::kWave;
  hipLaunchKernelGGL(nmf::nmf_taxis_kernel, dim3((unsigned)((n_worlds + per_block - 1) / per_block)), dim3(nmf::kTaxisThreads), 0, (hipStream_t)stream,
                     A, reinterpret_cast<const int*>(centres_dev), reinterpret_cast<const float2*>(omm_dev), odor_dev, odor_gains_dev,
                     features_dev, bias_dev, drive_dev);
  HIP_OK(hipGetLastError());
  return 0;
}

// ---- path integration (nmf_odometry.hip) ----
// The shared coefficients and the per-world state; the batch lends its pose and sensor arrays to every update.
struct nmf_odometry {
  const nmf_batch* batch = nullptr;
  int n_worlds = 0;
  nmf::OdoArgs args{};
  nmf::OdoPtrs ptrs{};
  DevMem mem;
};

extern "C" size_t nmf_odometry_params_size(void) { return sizeof(nmf_odometry_params); }

extern "C" void nmf_odometry_destroy(nmf_odometry* O) {
  if (!O) return;
  O->mem.release();
  delete O;
}

extern "C" int nmf_odometry_reset(nmf_odometry* O, const uint8_t* mask_dev, const double* pose_dev, void* stream) {
  if (!O) return fail("nmf_odometry_reset: null integrator");
  if ((uintptr_t)pose_dev & 7) return fail("nmf_odometry_reset: pose must be 8-byte aligned");
  DEVICE_GUARD(O);
  hipLaunchKernelGGL(nmf::nmf_odometry_reset_kernel, dim3((unsigned)((6 * O->n_worlds + 255) / 256), (unsigned)O->args.window), dim3(256), 0,
                     (hipStream_t)stream, O->args, O->ptrs, mask_dev, pose_dev);
  HIP_OK(hipGetLastError());
  return 0;
}

static int fill_odometry(nmf_odometry* O, const nmf_odometry_params* p, const double* coef) {
  const nmf_batch* b = O->batch;
  if (p->window < 1 || p->window > 4096) return fail("nmf_odometry_create: window must be in 1..4096, got " + std::to_string(p->window));
  if (b->model->nsensor == 0 || !b->st.sensordata) return fail("nmf_odometry_create: the batch's model has no leg sensors (nsensor == 0)");
  if (b->widths[NMF_SENSORDATA] != 96)
    return fail("nmf_odometry_create: the batch's sensordata is " + std::to_string(b->widths[NMF_SENSORDATA]) + " wide, the update reads six leg sensors of 16 values");
  const int nseg = b->model->nseg;
  if (p->root_seg < 0 || p->root_seg >= nseg) return fail("nmf_odometry_create: root_seg " + std::to_string(p->root_seg) + " is outside the batch's " + std::to_string(nseg) + " segments");
  for (int l = 0; l < 6; ++l)
    if (p->tip_seg[l] < 0 || p->tip_seg[l] >= nseg) return fail("nmf_odometry_create: tip_seg[" + std::to_string(l) + "] = " + std::to_string(p->tip_seg[l]) + " is outside the batch's " + std::to_string(nseg) + " segments");
  for (int l = 0; l < 6; ++l)
    if (!(p->contact_force_threshold[l] >= 0.f) || !std::isfinite(p->contact_force_threshold[l]))
      return fail("nmf_odometry_create: contact_force_threshold[" + std::to_string(l) + "] must be finite and not negative");
  for (int c = 0; coef && c < 14; ++c)
    if (!std::isfinite(coef[c])) return fail("nmf_odometry_create: coefficient " + std::to_string(c) + " is not finite");
  nmf::OdoArgs& A = O->args;
  A.n_worlds = O->n_worlds; A.nseg = nseg; A.root_seg = p->root_seg; A.window = p->window;
  for (int l = 0; l < 6; ++l) { A.tip_seg[l] = p->tip_seg[l]; A.thr[l] = p->contact_force_threshold[l]; }
  A.inv_window = 1.0 / (double)p->window;
  const size_t n = (size_t)O->n_worlds;
  nmf::OdoPtrs& P = O->ptrs;
  P.seg_xpos = b->st.seg_xpos; P.seg_xquat = b->st.seg_xquat; P.sensordata = b->st.sensordata;
  P.coef = (const double*)O->mem.upload(coef, sizeof(double) * 14);
  P.count = (int*)O->mem.alloc(sizeof(int) * n);
  P.xprev = (float*)O->mem.alloc(sizeof(float) * 6 * n);
  P.cprev = (uint8_t*)O->mem.alloc(6 * n);
  P.total = (double*)O->mem.alloc(sizeof(double) * 6 * n);
  P.win = (double*)O->mem.alloc(sizeof(double) * 6 * n);
  P.heading = (double*)O->mem.alloc(sizeof(double) * n);
  P.position = (double*)O->mem.alloc(sizeof(double) * 2 * n);
  P.home = (double*)O->mem.alloc(sizeof(double) * 2 * n);
  P.ring = (double*)O->mem.alloc(sizeof(double) * 6 * n * (size_t)p->window);
  if (!O->mem.ok) return -1;
  if (nmf_odometry_reset(O, nullptr, nullptr, nullptr) != 0) return -1;
  HIP_OK(hipDeviceSynchronize());
  return 0;
}

extern "C" nmf_odometry* nmf_odometry_create(nmf_batch* b, const nmf_odometry_params* p, const double* coef) {
  if (!b || !p) { fail("nmf_odometry_create: null batch / params"); return nullptr; }
  return build_or_destroy(b->mem.device, "nmf_odometry_create", new nmf_odometry(), nmf_odometry_destroy, [&](nmf_odometry* O) {
    O->n_worlds = b->n_worlds; O->batch = b;
    return fill_odometry(O, p, coef);
  });
}

extern "C" void* nmf_odometry_field_ptr(nmf_odometry* O, int which, int32_t* width) {
  if (!O) { fail("nmf_odometry_field_ptr: null integrator"); return nullptr; }
  const nmf::OdoPtrs& P = O->ptrs;
  void* ptr[7] = {P.total, P.win, P.heading, P.position, P.home, P.count, const_cast<double*>(P.coef)};
  const int32_t w[7] = {6, 6, 1, 2, 2, 1, 14};
  if (which < 0 || which > 6) { fail("nmf_odometry_field_ptr: no such field"); return nullptr; }
  if (width) *width = w[which];
  return ptr[which];
}

// Pure stream-ordered work: one kernel launch.
extern "C" int nmf_odometry_update(nmf_odometry* O, void* stream) {
  if (!O) return fail("nmf_odometry_update: null integrator");
  DEVICE_GUARD(O);
  hipLaunchKernelGGL(nmf::nmf_odometry_update_kernel, dim3((unsigned)((O->n_worlds + nmf::kOdoWorlds - 1) / nmf::kOdoWorlds)), dim3(nmf::kOdoThreads),
                     0, (hipStream_t)stream, O->args, O->ptrs);
  HIP_OK(hipGetLastError());
  return 0;
}

// ---- motion vision (nmf_motion.hip) ----
// The shared pair list, the per-world filter state and the outputs.
struct nmf_motion {
  int n_worlds = 0;
  nmf::MotionArgs args{};
  nmf::MotionPtrs ptrs{};
  float* drive = nullptr;
  DevMem mem;
};

extern "C" size_t nmf_motion_params_size(void) { return sizeof(nmf_motion_params); }

extern "C" void nmf_motion_destroy(nmf_motion* M) {
  if (!M) return;
  M->mem.release();
  delete M;
}

extern "C" int nmf_motion_reset(nmf_motion* M, const uint8_t* mask_dev, void* stream) {
  if (!M) return fail("nmf_motion_reset: null handle");
  DEVICE_GUARD(M);
  hipLaunchKernelGGL(nmf::nmf_motion_reset_kernel, dim3((unsigned)((M->n_worlds + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     M->n_worlds, mask_dev, M->ptrs.fresh);
  HIP_OK(hipGetLastError());
  return 0;
}

static int fill_motion(nmf_motion* M, const nmf_motion_params* p, const int32_t* pairs, const float* weights, int n_pairs, int n_omm) {
  if (n_omm < 1 || n_omm > nmf::kMaxOmmatidia) return fail("nmf_motion_create: n_omm must be in 1..1024, got " + std::to_string(n_omm));
  if (n_pairs < 0 || n_pairs > nmf::kMotionMaxPairs) return fail("nmf_motion_create: n_pairs must be in 0..3072, got " + std::to_string(n_pairs));
  if (n_pairs > 0 && (!pairs || !weights)) return fail("nmf_motion_create: null pairs / weights");
  const float values[7] = {p->a_fast, p->a_slow, p->gain, p->delta, p->base, p->drive_min, p->drive_max};
  for (float v : values)
    if (!std::isfinite(v)) return fail("nmf_motion_create: a parameter is not finite");
  if (p->a_fast < 0.f || p->a_fast > 1.f || p->a_slow < 0.f || p->a_slow > 1.f) return fail("nmf_motion_create: a_fast and a_slow must be in [0, 1]");
  std::vector<int32_t> table((size_t)4 * (size_t)std::max(n_pairs, 1), 0);      // (a, b, bits of wx, bits of wy)
  for (int k = 0; k < n_pairs; ++k) {
    const int32_t a = pairs[2 * k], b = pairs[2 * k + 1];
    if (a < 0 || a >= n_omm || b < 0 || b >= n_omm)
      return fail("nmf_motion_create: pair " + std::to_string(k) + " = (" + std::to_string(a) + ", " + std::to_string(b) + ") is outside the retina's " + std::to_string(n_omm) + " ommatidia");
    if (a == b) return fail("nmf_motion_create: pair " + std::to_string(k) + " joins ommatidium " + std::to_string(a) + " to itself (a == b)");
    if (!std::isfinite(weights[2 * k]) || !std::isfinite(weights[2 * k + 1])) return fail("nmf_motion_create: the weight of pair " + std::to_string(k) + " is not finite");
    table[4 * (size_t)k] = a; table[4 * (size_t)k + 1] = b;
    std::memcpy(&table[4 * (size_t)k + 2], weights + 2 * k, 2 * sizeof(float));
  }
  nmf::MotionArgs& A = M->args;
  A.p = *p;
  A.n_worlds = M->n_worlds; A.n_omm = n_omm; A.n_pairs = n_pairs; A.den = 65536.0 * (double)n_pairs;
  const size_t n = (size_t)M->n_worlds, cells = n * 2 * (size_t)n_omm;
  nmf::MotionPtrs& P = M->ptrs;
  P.pairs = (const int4*)M->mem.upload(table.data(), sizeof(int32_t) * table.size());
  P.fast = (float*)M->mem.alloc(sizeof(float) * cells);
  P.slow = (float*)M->mem.alloc(sizeof(float) * cells);
  P.fresh = (uint8_t*)M->mem.alloc(n);
  P.sums = (int*)M->mem.alloc(sizeof(int) * 4 * n);
  P.flow = (float*)M->mem.alloc(sizeof(float) * 4 * n);
  P.rotation = (float*)M->mem.alloc(sizeof(float) * n);
  P.translation = (float*)M->mem.alloc(sizeof(float) * n);
  const std::vector<float> ones(2 * n, 1.f);
  M->drive = (float*)M->mem.upload(ones.data(), sizeof(float) * ones.size());
  if (!M->mem.ok) return -1;
  if (nmf_motion_reset(M, nullptr, nullptr) != 0) return -1;
  HIP_OK(hipDeviceSynchronize());
  return 0;
}

extern "C" nmf_motion* nmf_motion_create(nmf_batch* b, const nmf_motion_params* p, const int32_t* pairs_host, const float* weights_host,
                                         int n_pairs, int n_omm) {
  if (!b || !p) { fail("nmf_motion_create: null batch / params"); return nullptr; }
  return build_or_destroy(b->mem.device, "nmf_motion_create", new nmf_motion(), nmf_motion_destroy, [&](nmf_motion* M) {
    M->n_worlds = b->n_worlds;
    return fill_motion(M, p, pairs_host, weights_host, n_pairs, n_omm);
  });
}

extern "C" void* nmf_motion_field_ptr(nmf_motion* M, int which, int32_t* width) {
  if (!M) { fail("nmf_motion_field_ptr: null handle"); return nullptr; }
  const nmf::MotionPtrs& P = M->ptrs;
  void* ptr[8] = {P.fast, P.slow, P.sums, P.flow, P.rotation, P.translation, M->drive, P.fresh};
  const int32_t w[8] = {2 * M->args.n_omm, 2 * M->args.n_omm, 4, 4, 1, 1, 2, 1};
  if (which < 0 || which > 7) { fail("nmf_motion_field_ptr: no such field"); return nullptr; }
  if (width) *width = w[which];
  return ptr[which];
}

// Pure stream-ordered work: one kernel launch.
extern "C" int nmf_motion_update(nmf_motion* M, const float* omm_dev, const float* base_dev, float* drive_out_dev, void* stream) {
  if (!M) return fail("nmf_motion_update: null handle");
  if (!omm_dev) return fail("nmf_motion_update: null omm");
  if (!drive_out_dev) return fail("nmf_motion_update: null drive");
  if (((uintptr_t)omm_dev & 7) || ((uintptr_t)base_dev & 3) || ((uintptr_t)drive_out_dev & 3))
    return fail("nmf_motion_update: omm must be 8-byte, base and drive 4-byte aligned");
  DEVICE_GUARD(M);
  hipLaunchKernelGGL(nmf::nmf_motion_kernel, dim3((unsigned)((M->n_worlds + nmf::kMotionWorlds - 1) / nmf::kMotionWorlds)), dim3(nmf::kMotionThreads),
                     0, (hipStream_t)stream, M->args, M->ptrs, reinterpret_cast<const float2*>(omm_dev), base_dev, drive_out_dev);
  HIP_OK(hipGetLastError());
  return 0;
}

// ---- retinotopic visual network (nmf_visnet.hip) ----
// The shared network (tap list grouped by post type, neighbour table), the per-world state and the outputs.
struct nmf_visnet {
  int n_worlds = 0;
  nmf::VisArgs args{};
  nmf::VisPtrs ptrs{};
  const int4* taps = nullptr;                  // grouped by post type
  const unsigned int* tables = nullptr;        // per eye, uint16 pairs
  float* drive = nullptr;
  unsigned threads = 0, lds_bytes = 0;
  DevMem mem;
};

extern "C" size_t nmf_visnet_params_size(void) { return sizeof(nmf_visnet_params); }

extern "C" void nmf_visnet_destroy(nmf_visnet* V) {
  if (!V) return;
  V->mem.release();
  delete V;
}

extern "C" int nmf_visnet_reset(nmf_visnet* V, const uint8_t* mask_dev, void* stream) {
  if (!V) return fail("nmf_visnet_reset: null handle");
  DEVICE_GUARD(V);
  hipLaunchKernelGGL(nmf::nmf_visnet_reset_kernel, dim3((unsigned)((V->n_worlds + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     V->n_worlds, mask_dev, V->ptrs.fresh);
  HIP_OK(hipGetLastError());
  return 0;
}

static int fill_visnet(nmf_visnet* V, const nmf_visnet_params* p, const float* types, const int32_t* neighbours, const int32_t* edges,
                       const int32_t* taps, const float* tap_w) {
  const std::string who = "nmf_visnet_create: ";
  const int C = p->n_types, n_omm = p->n_omm, T = p->n_table, E = p->n_edges, K = p->n_taps;
  if (C < 1 || C > NMF_VISNET_MAX_TYPES) return fail(who + "n_types must be in 1..32, got " + std::to_string(C));
  if (n_omm < 1 || n_omm > nmf::kMaxOmmatidia) return fail(who + "n_omm must be in 1..1024, got " + std::to_string(n_omm));
  if (C * n_omm > NMF_VISNET_MAX_CELLS)
    return fail(who + "n_types x n_omm must be at most 24576 cells, got " + std::to_string(C) + " x " + std::to_string(n_omm) + " = " + std::to_string(C * n_omm));
  if (T < 1 || T > NMF_VISNET_MAX_TABLE) return fail(who + "n_table must be in 1..19, got " + std::to_string(T));
  if (E < 0 || E > NMF_VISNET_MAX_EDGES) return fail(who + "n_edges must be in 0..512, got " + std::to_string(E));
  if (K < 0 || K > NMF_VISNET_MAX_TAPS) return fail(who + "n_taps must be in 0..4096, got " + std::to_string(K));
  if (p->substeps < 1 || p->substeps > NMF_VISNET_MAX_SUBSTEPS) return fail(who + "substeps must be in 1..8, got " + std::to_string(p->substeps));
  if ((E > 0 && !edges) || (K > 0 && (!taps || !tap_w))) return fail(who + "null edges / taps / tap weights");
  const float values[5] = {p->gain, p->delta, p->base, p->drive_min, p->drive_max};
  for (float v : values)
    if (!std::isfinite(v)) return fail(who + "a parameter is not finite");
  static const char* const kConstant[5] = {"bias", "in_w[0]", "in_w[1]", "a", "steer_w"};
  for (int c = 0; c < C; ++c) {
    for (int f = 0; f < 5; ++f)
      if (!std::isfinite(types[5 * c + f])) return fail(who + kConstant[f] + " of type " + std::to_string(c) + " is not finite");
    if (!(types[5 * c + 3] > 0.f) || types[5 * c + 3] > 1.f) return fail(who + "a of type " + std::to_string(c) + " must be in (0, 1]");
  }
  // the neighbour table as uint16, a missing neighbour = n_omm (the +0 cell of every LDS row), padded to whole 32-bit words
  const size_t per_eye = ((size_t)T * (size_t)n_omm + 1) & ~(size_t)1;
  std::vector<uint16_t> table(2 * per_eye, (uint16_t)n_omm);
  for (int e = 0; e < 2; ++e)
    for (int t = 0; t < T; ++t)
      for (int i = 0; i < n_omm; ++i) {
        const int32_t j = neighbours[((size_t)e * T + t) * n_omm + i];
        if (j < -1 || j >= n_omm)
          return fail(who + "neighbours[" + std::to_string(e) + "][" + std::to_string(t) + "][" + std::to_string(i) + "] = " + std::to_string(j) + " is outside -1.." + std::to_string(n_omm - 1));
        table[(size_t)e * per_eye + (size_t)t * n_omm + i] = (uint16_t)(j < 0 ? n_omm : j);
      }
  for (int e = 0; e < E; ++e)
    for (int f = 0; f < 2; ++f)
      if (edges[2 * e + f] < 0 || edges[2 * e + f] >= C)
        return fail(who + "edge " + std::to_string(e) + " = (" + std::to_string(edges[2 * e]) + ", " + std::to_string(edges[2 * e + 1]) + ") is outside the network's " + std::to_string(C) + " types");
  for (int k = 0; k < K; ++k) {
    if (taps[2 * k] < 0 || taps[2 * k] >= E) return fail(who + "tap " + std::to_string(k) + " belongs to edge " + std::to_string(taps[2 * k]) + ", outside the network's " + std::to_string(E) + " edges");
    if (taps[2 * k + 1] < 0 || taps[2 * k + 1] >= T) return fail(who + "tap " + std::to_string(k) + " reads row " + std::to_string(taps[2 * k + 1]) + ", outside the table's " + std::to_string(T) + " rows");
    if (!std::isfinite(tap_w[k])) return fail(who + "the weight of tap " + std::to_string(k) + " is not finite");
  }
  nmf::VisArgs& A = V->args;
  A.p = *p;
  A.n_worlds = V->n_worlds; A.n_omm = n_omm; A.n_types = C; A.n_table = T; A.substeps = p->substeps;
  A.row = n_omm + 1; A.nb_word = C * A.row; A.nb_words = (int)(per_eye / 2); A.part_word = A.nb_word + A.nb_words;
  A.den = 65536.0 * (double)n_omm;
  // the taps grouped by post type: the edges into a type in the caller's order, the taps of an edge in the caller's order
  std::vector<int32_t> flat((size_t)4 * (size_t)std::max(K, 1), 0);
  int count = 0;
  for (int c = 0; c < NMF_VISNET_MAX_TYPES; ++c) {
    A.start[c] = count;
    const bool used = c < C;
    A.bias[c] = used ? types[5 * c] : 0.f; A.in_w0[c] = used ? types[5 * c + 1] : 0.f; A.in_w1[c] = used ? types[5 * c + 2] : 0.f;
    A.a[c] = used ? types[5 * c + 3] : 0.f; A.steer_w[c] = used ? types[5 * c + 4] : 0.f;
    for (int e = 0; used && e < E; ++e) {
      if (edges[2 * e] != c) continue;
      for (int k = 0; k < K; ++k) {
        if (taps[2 * k] != e) continue;
        int32_t* out = &flat[4 * (size_t)count++];
        out[0] = edges[2 * e + 1] * A.row; out[1] = taps[2 * k + 1] * n_omm;
        std::memcpy(&out[2], &tap_w[k], sizeof(float));
      }
    }
  }
  A.start[NMF_VISNET_MAX_TYPES] = count;
  V->threads = (unsigned)((n_omm + nmf::kWave - 1) / nmf::kWave * nmf::kWave);
  V->lds_bytes = (unsigned)(sizeof(float) * ((size_t)A.part_word + (size_t)(V->threads / nmf::kWave) * NMF_VISNET_MAX_TYPES));
  if (V->lds_bytes > 64u * 1024u)
    HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(&nmf::nmf_visnet_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)(sizeof(float) * (NMF_VISNET_MAX_CELLS + NMF_VISNET_MAX_TYPES + (NMF_VISNET_MAX_TABLE * nmf::kMaxOmmatidia) / 2 +
                                                      (nmf::kVisMaxThreads / nmf::kWave) * NMF_VISNET_MAX_TYPES))));
  const size_t n = (size_t)V->n_worlds;
  nmf::VisPtrs& P = V->ptrs;
  V->taps = (const int4*)V->mem.upload(flat.data(), sizeof(int32_t) * flat.size());
  V->tables = (const unsigned int*)V->mem.upload(table.data(), sizeof(uint16_t) * table.size());
  P.v = (float*)V->mem.alloc(sizeof(float) * n * 2 * (size_t)C * (size_t)n_omm);
  P.fresh = (uint8_t*)V->mem.alloc(2 * n);
  P.sums = (int*)V->mem.alloc(sizeof(int) * n * 2 * (size_t)C);
  P.pooled = (float*)V->mem.alloc(sizeof(float) * n * 2 * (size_t)C);
  P.signal = (float*)V->mem.alloc(sizeof(float) * n);
  const std::vector<float> ones(2 * n, 1.f);
  V->drive = (float*)V->mem.upload(ones.data(), sizeof(float) * ones.size());
  if (!V->mem.ok) return -1;
  if (nmf_visnet_reset(V, nullptr, nullptr) != 0) return -1;
  HIP_OK(hipDeviceSynchronize());
  return 0;
}

extern "C" nmf_visnet* nmf_visnet_create(nmf_batch* b, const nmf_visnet_params* p, const float* types_host, const int32_t* neighbours_host,
                                         const int32_t* edges_host, const int32_t* taps_host, const float* tap_w_host) {
  if (!b || !p || !types_host || !neighbours_host) { fail("nmf_visnet_create: null batch / params / types / neighbours"); return nullptr; }
  return build_or_destroy(b->mem.device, "nmf_visnet_create", new nmf_visnet(), nmf_visnet_destroy, [&](nmf_visnet* V) {
    V->n_worlds = b->n_worlds;
    return fill_visnet(V, p, types_host, neighbours_host, edges_host, taps_host, tap_w_host);
  });
}

extern "C" void* nmf_visnet_field_ptr(nmf_visnet* V, int which, int32_t* width) {
  if (!V) { fail("nmf_visnet_field_ptr: null handle"); return nullptr; }
  const nmf::VisPtrs& P = V->ptrs;
  const int C = V->args.n_types;
  void* ptr[6] = {P.v, P.pooled, P.sums, P.signal, V->drive, P.fresh};
  const int32_t w[6] = {2 * C * V->args.n_omm, 2 * C, 2 * C, 1, 2, 2};
  if (which < 0 || which > 5) { fail("nmf_visnet_field_ptr: no such field"); return nullptr; }
  if (width) *width = w[which];
  return ptr[which];
}

// Pure stream-ordered work: two kernel launches.
extern "C" int nmf_visnet_update(nmf_visnet* V, const float* omm_dev, const float* base_dev, float* drive_out_dev, void* stream) {
  if (!V) return fail("nmf_visnet_update: null handle");
  if (!omm_dev) return fail("nmf_visnet_update: null omm");
  if (!drive_out_dev) return fail("nmf_visnet_update: null drive");
  if (((uintptr_t)omm_dev & 7) || ((uintptr_t)base_dev & 3) || ((uintptr_t)drive_out_dev & 3))
    return fail("nmf_visnet_update: omm must be 8-byte, base and drive 4-byte aligned");
  DEVICE_GUARD(V);
  hipLaunchKernelGGL(nmf::nmf_visnet_kernel, dim3(2u * (unsigned)V->n_worlds), dim3(V->threads), V->lds_bytes, (hipStream_t)stream,
                     V->args, V->ptrs, V->taps, V->tables, reinterpret_cast<const float2*>(omm_dev));
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(nmf::nmf_visnet_world_kernel, dim3((unsigned)((V->n_worlds + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     V->args, V->ptrs, base_dev, drive_out_dev);
  HIP_OK(hipGetLastError());
  return 0;
}

// ---- the walking task (nmf_task.hip) ----
// The per-world arrays and the handle's tables; the batch lends its pose, velocity, force, sensor and joint-angle arrays to every update.
struct nmf_task {
  int n_worlds = 0;
  nmf::TaskArgs args{};
  nmf::TaskPtrs ptrs{};
  DevMem mem;
};

extern "C" size_t nmf_task_params_size(void) { return sizeof(nmf_task_params); }

extern "C" void nmf_task_destroy(nmf_task* T) {
  if (!T) return;
  T->mem.release();
  delete T;
}

extern "C" int nmf_task_reset(nmf_task* T, const uint8_t* mask_dev, void* stream) {
  if (!T) return fail("nmf_task_reset: null task");
  DEVICE_GUARD(T);
  hipLaunchKernelGGL(nmf::nmf_task_reset_kernel, dim3((unsigned)((T->n_worlds + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     T->args, T->ptrs, mask_dev);
  HIP_OK(hipGetLastError());
  return 0;
}

static int fill_task(nmf_task* T, const nmf_batch* b, const nmf_task_params* p, const int32_t* act, const int32_t* act_dof,
                     const int32_t* obs_dof, const float* mean, const float* inv_std) {
  const std::string who = "nmf_task_create: ";
  if (p->n_act < 1 || p->n_act > NMF_TASK_MAX_ACT) return fail(who + "n_act must be in 1..64, got " + std::to_string(p->n_act));
  if (p->n_q < 1 || p->n_q > NMF_TASK_MAX_Q) return fail(who + "n_q must be in 1..256, got " + std::to_string(p->n_q));
  const float values[21] = {p->cos_max_tilt, p->z_min, p->z_max, p->arena[0], p->arena[1], p->arena[2], p->arena[3], p->goal_radius2,
                            p->power_clip, p->thr2[0], p->thr2[1], p->thr2[2], p->thr2[3], p->thr2[4], p->thr2[5], p->alive,
                            p->w_progress, p->w_power, p->w_tilt, p->bonus_goal, p->penalty_fail};
  for (float v : values)
    if (!std::isfinite(v)) return fail(who + "a parameter is not finite");
  for (int k = 0; k < p->n_q; ++k)
    if (!std::isfinite(mean[k]) || !std::isfinite(inv_std[k])) return fail(who + "mean or inv_std is not finite at input " + std::to_string(k));
  const int nseg = b->model->nseg, n_dof = b->model->nq - 7, nu = b->model->nu;
  if (p->root_seg < 0 || p->root_seg >= nseg) return fail(who + "root_seg " + std::to_string(p->root_seg) + " is outside the batch's " + std::to_string(nseg) + " segments");
  for (int a = 0; a < p->n_act; ++a) {
    if (act[a] < 0 || act[a] >= nu)
      return fail(who + "act[" + std::to_string(a) + "] = " + std::to_string(act[a]) + " is outside the model's " + std::to_string(nu) + " controls (nu)");
    if (act_dof[a] < 0 || act_dof[a] >= n_dof)
      return fail(who + "act_dof[" + std::to_string(a) + "] = " + std::to_string(act_dof[a]) + " is outside the model's " + std::to_string(n_dof) + " joint dofs");
  }
  for (int k = 0; k < p->n_q; ++k)
    if (obs_dof[k] < 0 || obs_dof[k] >= n_dof)
      return fail(who + "obs_dof[" + std::to_string(k) + "] = " + std::to_string(obs_dof[k]) + " is outside the model's " + std::to_string(n_dof) + " joint dofs");
  if (p->tilt_ticks < 1) return fail(who + "tilt_ticks must be at least 1, got " + std::to_string(p->tilt_ticks));
  if (p->airborne_ticks < 1) return fail(who + "airborne_ticks must be at least 1, got " + std::to_string(p->airborne_ticks));
  if (p->max_ticks < 1) return fail(who + "max_ticks must be at least 1, got " + std::to_string(p->max_ticks));
  if (p->grace_ticks < 0) return fail(who + "grace_ticks must not be negative, got " + std::to_string(p->grace_ticks));
  if (p->cos_max_tilt < -1.f || p->cos_max_tilt > 1.f) return fail(who + "cos_max_tilt must be in [-1, 1]");
  if (p->z_min > p->z_max) return fail(who + "z_min > z_max");
  if (!(p->arena[0] < p->arena[1]) || !(p->arena[2] < p->arena[3])) return fail(who + "the arena is empty: it takes x_min < x_max and y_min < y_max");
  if (p->goal_radius2 < 0.f) return fail(who + "goal_radius2 must not be negative");
  for (int l = 0; l < 6; ++l)
    if (p->thr2[l] < 0.f) return fail(who + "thr2 must not be negative at leg " + std::to_string(l));
  // the int32 power sum: n_act terms of at most rint(power_clip 2^k)
  const double top = std::nearbyint((double)(p->power_clip * (float)(1 << NMF_TASK_POWER_BITS)));
  if (p->power_clip < 0.f || top * (double)p->n_act > 2147483647.0)
    return fail(who + "power_clip must be in 0.." + std::to_string(2147483647.0 / (double)p->n_act / (double)(1 << NMF_TASK_POWER_BITS)) +
                " for " + std::to_string(p->n_act) + " actuators (the power sum is an int32 in units of 2^-" + std::to_string(NMF_TASK_POWER_BITS) + ")");
  if (b->model->nsensor == 0 || !b->st.sensordata || b->widths[NMF_SENSORDATA] != 96)
    return fail(who + "the contact flags need six leg sensors of 16 values, the batch's sensordata is " + std::to_string(b->widths[NMF_SENSORDATA]) + " wide");
  nmf::TaskArgs& A = T->args;
  A.p = *p;
  A.n_worlds = T->n_worlds; A.nseg = nseg; A.nq = b->widths[NMF_QPOS]; A.nv = b->widths[NMF_QVEL]; A.nu = b->widths[NMF_ACTUATOR_FORCE];
  A.sens_stride = b->widths[NMF_SENSORDATA]; A.obs_width = NMF_TASK_OBS_BODY + 6 + p->n_q;
  const size_t n = (size_t)T->n_worlds;
  nmf::TaskPtrs& P = T->ptrs;
  P.seg_xpos = b->st.seg_xpos; P.seg_xquat = b->st.seg_xquat; P.qpos = b->st.qpos; P.qvel = b->st.qvel;
  P.actuator_force = b->st.actuator_force; P.sensordata = b->st.sensordata;
  P.act = (const int*)T->mem.upload(act, sizeof(int) * (size_t)p->n_act);
  P.act_dof = (const int*)T->mem.upload(act_dof, sizeof(int) * (size_t)p->n_act);
  P.obs_dof = (const int*)T->mem.upload(obs_dof, sizeof(int) * (size_t)p->n_q);
  P.mean = (const float*)T->mem.upload(mean, sizeof(float) * (size_t)p->n_q);
  P.inv_std = (const float*)T->mem.upload(inv_std, sizeof(float) * (size_t)p->n_q);
  P.reward = (float*)T->mem.alloc(sizeof(float) * n);
  P.obs = (float*)T->mem.alloc(sizeof(float) * n * (size_t)A.obs_width);
  P.ep_return = (float*)T->mem.alloc(sizeof(float) * n);
  P.last_return = (float*)T->mem.alloc(sizeof(float) * n);
  P.prev_xy = (float*)T->mem.alloc(sizeof(float) * 2 * n);
  std::vector<float> course(2 * n, 0.f);
  for (size_t w = 0; w < n; ++w) course[2 * w] = 1.f;
  P.course = (float*)T->mem.upload(course.data(), sizeof(float) * 2 * n);
  P.goal = (float*)T->mem.alloc(sizeof(float) * 2 * n);
  P.terminated = (uint8_t*)T->mem.alloc(n); P.truncated = (uint8_t*)T->mem.alloc(n);
  P.done = (uint8_t*)T->mem.alloc(n); P.fresh = (uint8_t*)T->mem.alloc(n);
  int** words[8] = {&P.reason, &P.ep_length, &P.last_length, &P.last_reason, &P.tilt_count, &P.airborne_count, &P.episodes, &P.successes};
  for (int** slot : words) *slot = (int*)T->mem.alloc(sizeof(int) * n);
  if (!T->mem.ok) return -1;
  if (nmf_task_reset(T, nullptr, nullptr) != 0) return -1;
  HIP_OK(hipDeviceSynchronize());
  return 0;
}

extern "C" nmf_task* nmf_task_create(nmf_batch* b, const nmf_task_params* p, const int32_t* act, const int32_t* act_dof,
                                     const int32_t* obs_dof, const float* mean, const float* inv_std) {
  if (!b || !p || !act || !act_dof || !obs_dof || !mean || !inv_std) { fail("nmf_task_create: null batch / params / act / act_dof / obs_dof / mean / inv_std"); return nullptr; }
  return build_or_destroy(b->mem.device, "nmf_task_create", new nmf_task(), nmf_task_destroy, [&](nmf_task* T) {
    T->n_worlds = b->n_worlds;
    return fill_task(T, b, p, act, act_dof, obs_dof, mean, inv_std);
  });
}

extern "C" void* nmf_task_field_ptr(nmf_task* T, int which, int32_t* width) {
  if (!T) { fail("nmf_task_field_ptr: null task"); return nullptr; }
  const nmf::TaskPtrs& P = T->ptrs;
  void* ptr[NMF_TASK_FIELD_COUNT] = {P.reward, P.obs, P.ep_return, P.last_return, P.prev_xy, P.course, P.goal, P.terminated, P.truncated, P.done,
                                     P.fresh, P.reason, P.ep_length, P.last_length, P.last_reason, P.tilt_count, P.airborne_count, P.episodes,
                                     P.successes};
  if (which < 0 || which >= NMF_TASK_FIELD_COUNT) { fail("nmf_task_field_ptr: no such field"); return nullptr; }
  if (width) *width = which == NMF_TASK_OBS ? T->args.obs_width : (which >= NMF_TASK_PREV_XY && which <= NMF_TASK_GOAL_XY) ? 2 : 1;
  return ptr[which];
}

// Pure stream-ordered work: one kernel launch.
extern "C" int nmf_task_update(nmf_task* T, void* stream) {
  if (!T) return fail("nmf_task_update: null task");
  DEVICE_GUARD(T);
  hipLaunchKernelGGL(nmf::nmf_task_update_kernel, dim3((unsigned)((T->n_worlds + nmf::kTaskWorlds - 1) / nmf::kTaskWorlds)), dim3(nmf::kTaskThreads),
                     0, (hipStream_t)stream, T->args, T->ptrs);
  HIP_OK(hipGetLastError());
  return 0;
}

// ---- plume navigation (nmf_navigator.hip) ----
// The per-world state; the batch lends its seg_xquat array to every update.
struct nmf_navigator {
  int n_worlds = 0;
  nmf::NavArgs args{};
  nmf::NavPtrs ptrs{};
  DevMem mem;
};

extern "C" size_t nmf_navigator_params_size(void) { return sizeof(nmf_navigator_params); }

extern "C" void nmf_navigator_destroy(nmf_navigator* N) {
  if (!N) return;
  N->mem.release();
  delete N;
}

extern "C" int nmf_navigator_reset(nmf_navigator* N, const uint8_t* mask_dev, void* stream) {
  if (!N) return fail("nmf_navigator_reset: null navigator");
  DEVICE_GUARD(N);
  hipLaunchKernelGGL(nmf::nmf_navigator_reset_kernel, dim3((unsigned)((N->n_worlds + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     N->args, N->ptrs, mask_dev);
  HIP_OK(hipGetLastError());
  return 0;
}

static int fill_navigator(nmf_navigator* N, const nmf_batch* b, const nmf_navigator_params* p) {
  const float values[21] = {p->dt, p->threshold, p->decay_stop, p->decay_walk, p->decay_freq, p->inv_tau_freq, p->lambda_ws0, p->dlambda_ws,
                            p->lambda_sw0, p->dlambda_sw, p->lambda_turn, p->p_up0, p->up_gain, p->p_up_min, p->p_up_max,
                            p->walk_drive[0], p->walk_drive[1], p->stop_drive[0], p->stop_drive[1], p->turn_drive[0], p->turn_drive[1]};
  for (float v : values)
    if (!std::isfinite(v)) return fail("nmf_navigator_create: a parameter is not finite");
  if (p->threshold < 0.f) return fail("nmf_navigator_create: threshold must not be negative");
  const float decays[3] = {p->decay_stop, p->decay_walk, p->decay_freq};
  for (float d : decays)
    if (d < 0.f || d > 1.f) return fail("nmf_navigator_create: decay_stop, decay_walk and decay_freq must be in [0, 1]");
  if (p->p_up_min < 0.f || p->p_up_max > 1.f || p->p_up_min > p->p_up_max)
    return fail("nmf_navigator_create: p_up_min and p_up_max must be in [0, 1] with p_up_min <= p_up_max");
  if (p->turn_ticks < 1 || p->turn_ticks > 65535) return fail("nmf_navigator_create: turn_ticks must be in 1..65535, got " + std::to_string(p->turn_ticks));
  const int nseg = b->model->nseg;
  if (p->root_seg < 0 || p->root_seg >= nseg) return fail("nmf_navigator_create: root_seg " + std::to_string(p->root_seg) + " is outside the batch's " + std::to_string(nseg) + " segments");
  if (p->odor_dim < 0 || p->odor_dim > 7) return fail("nmf_navigator_create: odor_dim must be in 0..7, got " + std::to_string(p->odor_dim));
  if (p->first_world < 0) return fail("nmf_navigator_create: first_world must not be negative");
  nmf::NavArgs& A = N->args;
  A.p = *p;
  A.n_worlds = N->n_worlds; A.nseg = nseg;
  const size_t n = (size_t)N->n_worlds;
  nmf::NavPtrs& P = N->ptrs;
  P.seg_xquat = b->st.seg_xquat;
  P.state = (int*)N->mem.alloc(sizeof(int) * n);
  P.remaining = (int*)N->mem.alloc(sizeof(int) * n);
  P.above = (uint8_t*)N->mem.alloc(n);
  P.k_stop = (float*)N->mem.alloc(sizeof(float) * n);
  P.k_walk = (float*)N->mem.alloc(sizeof(float) * n);
  P.freq = (float*)N->mem.alloc(sizeof(float) * n);
  P.ticks = (unsigned int*)N->mem.alloc(sizeof(unsigned int) * n);
  P.encounters = (int*)N->mem.alloc(sizeof(int) * n);
  P.drive = (float*)N->mem.alloc(sizeof(float) * 2 * n);
  if (!N->mem.ok) return -1;
  if (nmf_navigator_reset(N, nullptr, nullptr) != 0) return -1;
  HIP_OK(hipDeviceSynchronize());
  return 0;
}

extern "C" nmf_navigator* nmf_navigator_create(nmf_batch* b, const nmf_navigator_params* p) {
  if (!b || !p) { fail("nmf_navigator_create: null batch / params"); return nullptr; }
  return build_or_destroy(b->mem.device, "nmf_navigator_create", new nmf_navigator(), nmf_navigator_destroy, [&](nmf_navigator* N) {
    N->n_worlds = b->n_worlds;
    return fill_navigator(N, b, p);
  });
}

extern "C" void* nmf_navigator_field_ptr(nmf_navigator* N, int which, int32_t* width) {
  if (!N) { fail("nmf_navigator_field_ptr: null navigator"); return nullptr; }
  const nmf::NavPtrs& P = N->ptrs;
  void* ptr[9] = {P.state, P.remaining, P.above, P.k_stop, P.k_walk, P.freq, P.ticks, P.encounters, P.drive};
  if (which < 0 || which > 8) { fail("nmf_navigator_field_ptr: no such field"); return nullptr; }
  if (width) *width = which == NMF_NAVIGATOR_DRIVE ? 2 : 1;
  return ptr[which];
}

// Pure stream-ordered work: one kernel launch.
extern "C" int nmf_navigator_update(nmf_navigator* N, const float* odor_dev, int n_dims, const float* wind_dev, int wind_rows,
                                    float* drive_out_dev, void* stream) {
  if (!N) return fail("nmf_navigator_update: null navigator");
  if (!odor_dev) return fail("nmf_navigator_update: null odor");
  if (!wind_dev) return fail("nmf_navigator_update: null wind");
  if (n_dims <= N->args.p.odor_dim)
    return fail("nmf_navigator_update: odor has " + std::to_string(n_dims) + " dimensions, the navigator reads dimension " + std::to_string(N->args.p.odor_dim));
  if (wind_rows != 1 && wind_rows != N->n_worlds)
    return fail("nmf_navigator_update: wind_rows must be 1 or " + std::to_string(N->n_worlds) + " (n_worlds), got " + std::to_string(wind_rows));
  if (((uintptr_t)odor_dev & 15) || ((uintptr_t)wind_dev & 3) || ((uintptr_t)drive_out_dev & 7))
    return fail("nmf_navigator_update: odor must be 16-byte, wind 4-byte and drive 8-byte aligned");
  DEVICE_GUARD(N);
  hipLaunchKernelGGL(nmf::nmf_navigator_update_kernel, dim3((unsigned)((N->n_worlds + nmf::kNavThreads - 1) / nmf::kNavThreads)), dim3(nmf::kNavThreads),
                     0, (hipStream_t)stream, N->args, N->ptrs, odor_dev, n_dims, wind_dev, wind_rows, drive_out_dev ? drive_out_dev : N->ptrs.drive);
  HIP_OK(hipGetLastError());
  return 0;
}

// ---- head stabilization (nmf_stabilizer.hip) ----
// The uploaded network and the handle's own output array; the batch lends its qpos, sensordata and ctrl arrays to every update.
struct nmf_stabilizer {
  int n_worlds = 0;
  nmf::StabArgs args{};
  const float* qpos = nullptr; const float* sensordata = nullptr; float* ctrl = nullptr;
  const int* dof = nullptr; const float* mean = nullptr; const float* inv_std = nullptr; const float* blob = nullptr;
  float* out = nullptr;
  unsigned lds_bytes = 0;
  DevMem mem;
};

extern "C" size_t nmf_stabilizer_params_size(void) { return sizeof(nmf_stabilizer_params); }

extern "C" void nmf_stabilizer_destroy(nmf_stabilizer* S) {
  if (!S) return;
  S->mem.release();
  delete S;
}

static int fill_stabilizer(nmf_stabilizer* S, const nmf_batch* b, const nmf_stabilizer_params* p, const int32_t* dof, const float* mean,
                           const float* inv_std, const float* weights, const int32_t* act) {
  const std::string who = "nmf_stabilizer_create: ";
  if (p->n_hidden < 1 || p->n_hidden > NMF_STABILIZER_MAX_HIDDEN)
    return fail(who + "n_hidden must be in 1..3, got " + std::to_string(p->n_hidden));
  for (int i = 0; i < p->n_hidden; ++i)
    if (p->hidden[i] < 1 || p->hidden[i] > NMF_STABILIZER_MAX_WIDTH)
      return fail(who + "hidden[" + std::to_string(i) + "] must be in 1..64, got " + std::to_string(p->hidden[i]));
  if (p->n_q < 1) return fail(who + "n_q must be at least 1, got " + std::to_string(p->n_q));
  const int n_in = p->n_q + (p->contacts ? 6 : 0);
  if (p->n_q > NMF_STABILIZER_MAX_IN || n_in > NMF_STABILIZER_MAX_IN) return fail(who + "n_in must be at most 256, got " + std::to_string(n_in));
  if (p->n_out < 1 || p->n_out > NMF_STABILIZER_MAX_OUT) return fail(who + "n_out must be in 1..8, got " + std::to_string(p->n_out));
  const int n_dof = b->model->nq - 7, nu = b->model->nu;
  for (int k = 0; k < p->n_q; ++k)
    if (dof[k] < 0 || dof[k] >= n_dof)
      return fail(who + "dof[" + std::to_string(k) + "] = " + std::to_string(dof[k]) + " is outside the model's " + std::to_string(n_dof) + " joint dofs");
  for (int j = 0; act && j < p->n_out; ++j)
    if (act[j] < 0 || act[j] >= nu)
      return fail(who + "act[" + std::to_string(j) + "] = " + std::to_string(act[j]) + " is outside the model's " + std::to_string(nu) + " controls (nu)");
  for (int j = 0; j < p->n_out; ++j) {
    if (!std::isfinite(p->lo[j]) || !std::isfinite(p->hi[j])) return fail(who + "a bound is not finite");
    if (p->lo[j] > p->hi[j]) return fail(who + "lo[" + std::to_string(j) + "] > hi[" + std::to_string(j) + "]");
  }
  for (int k = 0; k < p->n_q; ++k)
    if (!std::isfinite(mean[k]) || !std::isfinite(inv_std[k])) return fail(who + "mean or inv_std is not finite at input " + std::to_string(k));
  if (p->contacts) {
    for (int l = 0; l < 6; ++l)
      if (!std::isfinite(p->thr2[l])) return fail(who + "thr2 is not finite at leg " + std::to_string(l));
    if (b->model->nsensor == 0 || !b->st.sensordata || b->widths[NMF_SENSORDATA] != 96)
      return fail(who + "the contact flags need six leg sensors of 16 values, the batch's sensordata is " + std::to_string(b->widths[NMF_SENSORDATA]) + " wide");
  }
  nmf::StabArgs& A = S->args;
  A.n_worlds = S->n_worlds; A.qpos_stride = b->widths[NMF_QPOS]; A.sens_stride = b->widths[NMF_SENSORDATA]; A.ctrl_stride = b->widths[NMF_CTRL];
  A.n_q = p->n_q; A.n_in = n_in; A.contacts = p->contacts ? 1 : 0; A.n_layers = p->n_hidden + 1; A.drive = act ? 1 : 0;
  // the blob: per layer bias[jpad], then Wt[k][jpad], jpad = the width rounded up to a block, zeros in the padding
  std::vector<float> blob;
  const float* src = weights;
  int n_prev = n_in;
  for (int i = 0; i < A.n_layers; ++i) {
    const int width = i < p->n_hidden ? p->hidden[i] : p->n_out;
    const int jpad = (width + nmf::kStabBlock - 1) / nmf::kStabBlock * nmf::kStabBlock;
    const size_t count = (size_t)width * (size_t)n_prev + (size_t)width;
    for (size_t c = 0; c < count; ++c)
      if (!std::isfinite(src[c])) return fail(who + "a weight or bias of layer " + std::to_string(i) + " is not finite");
    A.width[i] = width; A.offset[i] = (int)blob.size();
    blob.resize(blob.size() + (size_t)jpad * (size_t)(n_prev + 1), 0.f);
    float* bias = blob.data() + A.offset[i];
    float* wt = bias + jpad;
    for (int j = 0; j < width; ++j) {
      bias[j] = src[(size_t)width * (size_t)n_prev + j];
      for (int k = 0; k < n_prev; ++k) wt[(size_t)k * jpad + j] = src[(size_t)j * n_prev + k];
    }
    src += count;
    n_prev = width;
  }
  // two LDS buffers of [unit][lane]: the inputs and the second hidden layer in the first, the other hidden layers in the second
  const int size_a = std::max(n_in, p->n_hidden >= 2 ? p->hidden[1] : 0);
  const int size_b = std::max(p->hidden[0], p->n_hidden >= 3 ? p->hidden[2] : 0);
  A.lds_b = size_a;
  S->lds_bytes = (unsigned)(sizeof(float) * nmf::kStabLanes * (size_t)(size_a + size_b));
  if (S->lds_bytes > 64u * 1024u)
    HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(&nmf::nmf_stabilizer_update_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)(sizeof(float) * nmf::kStabLanes * (NMF_STABILIZER_MAX_IN + NMF_STABILIZER_MAX_WIDTH))));
  for (int j = 0; j < NMF_STABILIZER_MAX_OUT; ++j) {
    const bool used = j < p->n_out;
    A.lo[j] = used ? p->lo[j] : 0.f; A.hi[j] = used ? p->hi[j] : 0.f; A.act[j] = used && act ? act[j] : 0;
  }
  for (int l = 0; l < 6; ++l) A.thr2[l] = p->contacts ? p->thr2[l] : 0.f;
  S->qpos = b->st.qpos; S->sensordata = b->st.sensordata; S->ctrl = b->st.ctrl;
  S->dof = (const int*)S->mem.upload(dof, sizeof(int) * (size_t)p->n_q);
  S->mean = (const float*)S->mem.upload(mean, sizeof(float) * (size_t)p->n_q);
  S->inv_std = (const float*)S->mem.upload(inv_std, sizeof(float) * (size_t)p->n_q);
  S->blob = (const float*)S->mem.upload(blob.data(), sizeof(float) * blob.size());
  S->out = (float*)S->mem.alloc(sizeof(float) * (size_t)S->n_worlds * (size_t)p->n_out);
  if (!S->mem.ok) return -1;
  return 0;
}

extern "C" nmf_stabilizer* nmf_stabilizer_create(nmf_batch* b, const nmf_stabilizer_params* p, const int32_t* dof, const float* mean,
                                                 const float* inv_std, const float* weights, const int32_t* act) {
  if (!b || !p || !dof || !mean || !inv_std || !weights) { fail("nmf_stabilizer_create: null batch / params / dof / mean / inv_std / weights"); return nullptr; }
  return build_or_destroy(b->mem.device, "nmf_stabilizer_create", new nmf_stabilizer(), nmf_stabilizer_destroy, [&](nmf_stabilizer* S) {
    S->n_worlds = b->n_worlds;
    return fill_stabilizer(S, b, p, dof, mean, inv_std, weights, act);
  });
}

extern "C" void* nmf_stabilizer_field_ptr(nmf_stabilizer* S, int which, int32_t* width) {
  if (!S) { fail("nmf_stabilizer_field_ptr: null stabilizer"); return nullptr; }
  if (which != NMF_STABILIZER_OUTPUT) { fail("nmf_stabilizer_field_ptr: no such field"); return nullptr; }
  if (width) *width = S->args.width[S->args.n_layers - 1];
  return S->out;
}

// Pure stream-ordered work: one kernel launch.
extern "C" int nmf_stabilizer_update(nmf_stabilizer* S, float* out_dev, void* stream) {
  if (!S) return fail("nmf_stabilizer_update: null stabilizer");
  if ((uintptr_t)out_dev & 15) return fail("nmf_stabilizer_update: out must be 16-byte aligned");
  DEVICE_GUARD(S);
  hipLaunchKernelGGL(nmf::nmf_stabilizer_update_kernel, dim3((unsigned)((S->n_worlds + nmf::kStabLanes - 1) / nmf::kStabLanes)), dim3(nmf::kStabLanes * nmf::kStabWaves),
                     S->lds_bytes, (hipStream_t)stream, S->args, S->qpos, S->sensordata, S->dof, S->mean, S->inv_std, S->blob, S->ctrl,
                     out_dev ? out_dev : S->out);
  HIP_OK(hipGetLastError());
  return 0;
}

// ---- rule-based walking (nmf_rules.hip) ----
// The controller's shared tables (own device copies) and its per-world state.
struct nmf_rules {
  int n_worlds = 0, table_steps = 0;
  nmf::RulesArgs args{};
  nmf::RulesPtrs ptrs{};
  DevMem mem;
};

extern "C" size_t nmf_rules_params_size(void) { return sizeof(nmf_rules_params); }

extern "C" void nmf_rules_destroy(nmf_rules* R) {
  if (!R) return;
  R->mem.release();
  delete R;
}

extern "C" int nmf_rules_reset(nmf_rules* R, const uint8_t* mask_dev, void* stream) {
  if (!R) return fail("nmf_rules_reset: null controller");
  DEVICE_GUARD(R);
  hipLaunchKernelGGL(nmf::nmf_rules_reset_kernel, dim3((unsigned)((6 * R->n_worlds + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     R->n_worlds, mask_dev, R->ptrs);
  HIP_OK(hipGetLastError());
  return 0;
}

static int fill_rules(nmf_rules* R, const nmf_rules_params* p, const float* cycle, const int32_t* leg_of_col, const int32_t* start_bin,
                      const int32_t* swing_steps, const float* weights) {
  const std::string who = "nmf_rules_create: ";
  if (p->n_pos < 1 || p->n_pos > 4096) return fail(who + "need 1 <= n_pos <= 4096 position columns");
  if (p->n_bins < 2 || p->n_bins > (1 << 20)) return fail(who + "need 2 <= n_bins <= 2^20 phase bins");
  if (p->table_steps < 1) return fail(who + "table_steps must be at least 1");
  if (p->period_steps < 2) return fail(who + "period_steps must be at least 2, got " + std::to_string(p->period_steps));
  if ((int64_t)p->period_steps * (int64_t)p->n_bins >= (int64_t)1 << 31)
    return fail(who + "period_steps * n_bins must be below 2^31, got " + std::to_string(p->period_steps) + " * " + std::to_string(p->n_bins));
  for (int c = 0; c < p->n_pos; ++c)
    if (leg_of_col[c] < 0 || leg_of_col[c] > 5) return fail(who + "leg_of_col[" + std::to_string(c) + "] is outside 0..5");
  for (int l = 0; l < 6; ++l) {
    if (start_bin[l] < 0 || start_bin[l] >= p->n_bins) return fail(who + "start_bin[" + std::to_string(l) + "] is outside 0 .. n_bins - 1");
    if (swing_steps[l] < 1 || swing_steps[l] >= p->period_steps)
      return fail(who + "swing_steps[" + std::to_string(l) + "] = " + std::to_string(swing_steps[l]) + " is outside 1 .. period_steps - 1");
  }
  for (int i = 0; i < 108; ++i)
    if (!std::isfinite(weights[i])) return fail(who + "a weight is not finite");
  const float values[4] = {p->margin, p->max_amplitude, p->adhesion_on, p->adhesion_off};
  for (float v : values)
    if (!std::isfinite(v)) return fail(who + "margin, max_amplitude or an adhesion value is not finite");
  if (p->margin < 0.f || p->max_amplitude < 0.f) return fail(who + "margin and max_amplitude must not be negative");
  if (p->first_world < 0) return fail(who + "first_world must not be negative");
  nmf::RulesArgs& A = R->args;
  A.n_worlds = R->n_worlds; A.n_pos = p->n_pos; A.n_act = p->n_pos + (p->adhesion ? 6 : 0); A.n_bins = p->n_bins; A.period = p->period_steps;
  A.margin = p->margin; A.max_amplitude = p->max_amplitude; A.adhesion_on = p->adhesion_on; A.adhesion_off = p->adhesion_off;
  A.seed = p->seed; A.first_world = p->first_world;
  R->table_steps = p->table_steps;
  std::vector<float> rest((size_t)p->n_pos);
  for (int c = 0; c < p->n_pos; ++c) rest[(size_t)c] = cycle[(size_t)start_bin[leg_of_col[c]] * p->n_pos + c];
  const size_t n = (size_t)R->n_worlds;
  nmf::RulesPtrs& P = R->ptrs;
  P.cycle = (const float*)R->mem.upload(cycle, sizeof(float) * (size_t)p->n_bins * (size_t)p->n_pos);
  P.rest = (const float*)R->mem.upload(rest.data(), sizeof(float) * rest.size());
  P.leg_of_col = (const int*)R->mem.upload(leg_of_col, sizeof(int) * (size_t)p->n_pos);
  P.start_bin = (const int*)R->mem.upload(start_bin, sizeof(int) * 6);
  P.swing_steps = (const int*)R->mem.upload(swing_steps, sizeof(int) * 6);
  P.weights = (const float*)R->mem.upload(weights, sizeof(float) * 108);
  P.counter = (int*)R->mem.alloc(sizeof(int) * 6 * n);
  P.stepping = (uint8_t*)R->mem.alloc(6 * n);
  P.amplitude = (float*)R->mem.alloc(sizeof(float) * 6 * n);
  P.drive = (float*)R->mem.alloc(sizeof(float) * 2 * n);
  P.ticks = (unsigned int*)R->mem.alloc(sizeof(unsigned int) * n);
  P.scores = (float*)R->mem.alloc(sizeof(float) * 6 * n);
  if (!R->mem.ok) return -1;
  if (nmf_rules_reset(R, nullptr, nullptr) != 0) return -1;
  HIP_OK(hipDeviceSynchronize());
  return 0;
}

extern "C" nmf_rules* nmf_rules_create(nmf_batch* b, const nmf_rules_params* p, const float* cycle, const int32_t* leg_of_col,
                                       const int32_t* start_bin, const int32_t* swing_steps, const float* weights) {
  if (!b || !p) { fail("nmf_rules_create: null batch / params"); return nullptr; }
  if (!cycle || !leg_of_col || !start_bin || !swing_steps || !weights) {
    fail("nmf_rules_create: cycle, leg_of_col, start_bin, swing_steps and weights are required"); return nullptr;
  }
  return build_or_destroy(b->mem.device, "nmf_rules_create", new nmf_rules(), nmf_rules_destroy, [&](nmf_rules* R) {
    R->n_worlds = b->n_worlds;
    return fill_rules(R, p, cycle, leg_of_col, start_bin, swing_steps, weights);
  });
}

extern "C" void* nmf_rules_field_ptr(nmf_rules* R, int which, int32_t* width) {
  if (!R) { fail("nmf_rules_field_ptr: null controller"); return nullptr; }
  const nmf::RulesPtrs& P = R->ptrs;
  void* ptr[6] = {P.counter, P.stepping, P.amplitude, P.drive, P.ticks, P.scores};
  const int32_t w[6] = {6, 6, 6, 2, 1, 6};
  if (which < 0 || which > 5) { fail("nmf_rules_field_ptr: no such field"); return nullptr; }
  if (width) *width = w[which];
  return ptr[which];
}

// Pure stream-ordered work: argument checks on the host, one kernel launch.
extern "C" int nmf_rules_advance(nmf_rules* R, int n_steps, float* table_dev, int table_steps, void* stream) {
  const std::string w = "nmf_rules_advance";
  if (!R) return fail(w + ": null controller");
  DEVICE_GUARD(R);
  if (check_table(w, R->table_steps, R->mem.device, n_steps, table_dev, table_steps, stream) != 0) return -1;
  hipLaunchKernelGGL(nmf::nmf_rules_advance_kernel, dim3((unsigned)((R->n_worlds + nmf::kRulesWorlds - 1) / nmf::kRulesWorlds)), dim3(nmf::kRulesThreads),
                     0, (hipStream_t)stream, R->args, R->ptrs, table_dev, table_steps, n_steps);
  HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int nmf_odor_intensity(nmf_batch* b, const int32_t* sensor_seg_dev, const float* sensor_rel_dev, int n_sensors,
                                  const float* source_pos_dev, const float* source_peak_dev, int n_sources, int n_dims,
                                  float* out_dev, void* stream) {
  if (!b) return fail("nmf_odor_intensity: null batch");
  if (n_sensors <= 0 || n_sources < 0 || n_dims <= 0 || !sensor_seg_dev || !sensor_rel_dev || !out_dev)
    return fail("nmf_odor_intensity: bad arguments");
  int total = b->n_worlds * n_sensors;
  DEVICE_GUARD(b);
  hipLaunchKernelGGL(nmf::nmf_odor_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     b->st.seg_xpos, b->st.seg_xquat, b->model->nseg, sensor_seg_dev, sensor_rel_dev, n_sensors,
                     source_pos_dev, source_peak_dev, n_sources, n_dims, out_dev, b->n_worlds);
  HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int nmf_replay_resample(const float* clip_dev, int n_frames, int n_cols, double fps, double out_dt,
                                   const double* sg_taps_dev, int window, int n_out, float* out_dev, void* stream) {
  if (!clip_dev || !sg_taps_dev || !out_dev) return fail("nmf_replay_resample: null buffer");
  if (n_frames < 6 || n_frames > nmf::kReplayMaxFrames) return fail("nmf_replay_resample: need 6 <= n_frames <= 1536");
  if (window < 3 || !(window & 1) || window > n_frames) return fail("nmf_replay_resample: the filter window must be odd, >= 3 and <= n_frames");
  if (n_cols <= 0 || n_out <= 0 || !(fps > 0.0) || !(out_dt > 0.0)) return fail("nmf_replay_resample: bad sizes / rates");
  hipLaunchKernelGGL(nmf::nmf_replay_resample_kernel, dim3((unsigned)n_cols), dim3(nmf::kReplayThreads), 0, (hipStream_t)stream,
                     clip_dev, n_frames, n_cols, fps, out_dt, sg_taps_dev, window, n_out, out_dev);
  HIP_OK(hipGetLastError());
  return 0;
}

#ifdef NMF_SCHED_TRACE
// diagnostic build only: per-workgroup schedule trace of the last stepping launch (see nmf_step_diag.h)
extern "C" int nmf_debug_sched_trace(unsigned long long* out, int n_groups) {
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(nmf::g_sched_trace), sizeof(unsigned long long) * 8 * (size_t)std::min(n_groups, 4096)) != hipSuccess) return -1;
  return 0;
}
#endif

#ifdef NMF_STAGE_PROFILE
// diagnostic build only: cumulative s_memtime cycles per pipeline stage of wave 0
extern "C" int nmf_debug_stage_cycles(unsigned long long* out, int n, int reset) {
  unsigned long long host[NMF_NSTAGE] = {};
  if (hipMemcpyFromSymbol(host, HIP_SYMBOL(nmf::g_stage_cycles), sizeof(host)) != hipSuccess) return -1;
  for (int i = 0; i < n && i < NMF_NSTAGE; ++i) out[i] = host[i];
  if (reset) { unsigned long long z[NMF_NSTAGE] = {}; (void)hipMemcpyToSymbol(HIP_SYMBOL(nmf::g_stage_cycles), z, sizeof(z)); }
  return 0;
}
// diagnostic build only: the shared-prefix histogram of the contact-space solve's later eliminations (nmf_step_diag.h)
// (n: the words `out` holds; the call fails unless that is the histogram's size, returned when out is null)
extern "C" int nmf_debug_resume_hist(unsigned long long* out, int n, int reset) {
  if (!out) return NMF_RESUME_ROWS * 65;
  if (n != NMF_RESUME_ROWS * 65) return -1;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(nmf::g_resume_hist), sizeof(unsigned long long) * NMF_RESUME_ROWS * 65) != hipSuccess) return -1;
  if (reset) { static unsigned long long z[NMF_RESUME_ROWS * 65] = {}; (void)hipMemcpyToSymbol(HIP_SYMBOL(nmf::g_resume_hist), z, sizeof(z)); }
  return 0;
}
#endif
#ifdef NMF_EYE_STATS
extern "C" int nmf_debug_eye_stats(unsigned long long* out) {
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(nmf::g_eye_stats), sizeof(unsigned long long) * 8) != hipSuccess) return -1;
  unsigned long long z[8] = {};
  (void)hipMemcpyToSymbol(HIP_SYMBOL(nmf::g_eye_stats), z, sizeof(z));
  return 0;
}
#endif
#endif  // NMF_DEVMEM_CHECK
