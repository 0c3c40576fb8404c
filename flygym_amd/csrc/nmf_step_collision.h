// nmf_step_collision.h — collision stage: the terrain as height cells with side faces (terrain_*), then stage_collision — geoms
// against the ground plane or the terrain.  Reads the body poses (xmat / xpos overlays) and the model's hot part; leaves the
// step's contacts (c_r, c_D = distance, c_mu, c_info, body_cstart, ncon, overflow, nwall).  Its scratch (CollisionScratch, the
// geom slot table, the candidate list) is overlaid on T..W and, where that is too small, on the contact wrenches behind the
// positions.
//
// Not self-contained: one of the stage headers that nmf_step.hip includes in stage order to form the stepping kernel's
// translation unit, and it relies on the ones before it.
#pragma once
#include "nmf_device.h"

namespace nmf {

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

}  // namespace nmf
