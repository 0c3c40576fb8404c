// nmf_scene.h — the scene both ray casters look at (nmf_eyes.hip, nmf_camera.hip): checker ground or the terrain relief of the
// physics, sky, up to 8 spheres, flies as capsules.  One definition of what the two kernels do alike on a ray's path: the
// relief's cells and the walk of a ray through them, the flat ground hit, R * v, and two small helpers.  What differs on purpose stays in the two files: the ray-sphere and ray-capsule intersections, the lens and
// the pinhole, the capd layouts, the run sums and the tile output.
//
// THE RULE OF THIS HEADER: nothing on a ray's path may come from a header compiled without the pragma below.  The library is
// built with -fassociative-math, and fast-math flags sit on each instruction where it was WRITTEN: a helper of nmf_device.h
// (mat_vec, dot, the V3 operators, qmat) keeps re-associable adds when it is inlined into a renderer, and the pixel-exact and
// the sampled instantiation of the eye kernel must colour a pixel identically (tests/test_sensors.py) — which they only do if no
// sum of a ray's arithmetic may be re-associated differently in the two.  Measured (profiles/scene_header_digests.txt): the eye
// kernel's spelled-out R * v as rot3 below keeps the kernels' registers; the same products as mat_vec of nmf_device.h
// re-allocate every eye instantiation (71 -> 62 VGPRs, 10 -> 0 spilled registers, ...), i.e. another kernel.
// The known exception, NOT in this header: the per-workgroup staging of both kernels (the camera pose, a capsule's end points,
// the cover discs of spheres and capsule thirds) calls dot, the V3 operators, mat_vec and qmat of nmf_device.h and has from the
// start.  Moved into functions here (cover_disc / capsule_cover / capsule_ends) it changed the eye frames of all three relief
// worlds on the GPU (tests/test_render_bits_gpu.py), so it stays written out in the two files, four cover sites and two
// end-point sites.  Two more pieces were tried here and stay written out, each for a measured reason (same record): the
// cone-against-disc test of the culling (`meets`: as one function three kernels missed the speed bar by 0.6-1.0 %) and the
// eye kernel's relief walk (through relief_walk's callbacks the <false, true, true> instantiation spills a nineteenth register).
//
// The pragma holds from here to the end of the translation unit, whatever is included after this header (nmf_capi.hip).
#pragma once
#include "nmf_device.h"

#pragma clang fp reassociate(off)

namespace nmf {

constexpr int kMaxSpheres = 8;
constexpr int kMaxTerrainCells = 64;    // cells a ray is followed through the relief before the far field is taken as flat
constexpr float kTerrainEps = 1e-4f;    // the cell a ray is in at parameter t holds its point at t + eps (mm)
constexpr float kTerrainEpsRel = 4.76837158203125e-7f;   // ... and eps is no less than t * 2^-21: beyond t = 210 mm a float32 t + 1e-4 stops moving (the eye renderer)
constexpr float kTerrainWallTol = 1e-4f;   // entered through the side wall: this far below the cell's level (levels differ by >= 0.3 mm)

// constant-height cell of h(x, y) that holds (x, y): bounds (+-inf where unbounded) and level — the same arithmetic as
// the physics' terrain_height (nmf_step_collision.h) and as oracle/sensors_oracle.py::terrain_cell
struct TerrainCell { float x0, x1, y0, y1, h; };
__device__ __forceinline__ TerrainCell cell_gapped(float block, float gap, float depth, float x) {
  const float period = block + gap;
  const float base = floorf(x / period) * period;
  const bool on = x - base < block;
  return TerrainCell{on ? base : base + block, on ? base + block : base + period, -INFINITY, INFINITY, on ? 0.f : -depth};
}
__device__ __forceinline__ TerrainCell cell_blocks(float size, float height, float x, float y) {
  const float i = floorf(x / size), j = floorf(y / size);
  const float sum = i + j;
  const float par = sum - 2.f * floorf(sum / 2.f);
  return TerrainCell{i * size, (i + 1.f) * size, j * size, (j + 1.f) * size, par != 0.f ? height : 0.f};
}
__device__ __forceinline__ TerrainCell relief_cell(int kind, const float* p, float x, float y) {
  if (kind == 1) return cell_gapped(p[0], p[1], p[2], x);
  if (kind == 2) return cell_blocks(p[0], p[1], x, y);
  if (kind == 3) {
    const float st = floorf(x / p[3]);
    const float k = st - 3.f * floorf(st / 3.f);
    const float s0 = st * p[3], s1 = (st + 1.f) * p[3];
    if (k == 1.f) { TerrainCell c = cell_gapped(1.0f, p[1], p[2], x); c.x0 = fmaxf(c.x0, s0); c.x1 = fminf(c.x1, s1); return c; }
    if (k == 2.f) { TerrainCell c = cell_blocks(p[0], 0.35f, x, y); c.x0 = fmaxf(c.x0, s0); c.x1 = fminf(c.x1, s1); return c; }
    return TerrainCell{s0, s1, -INFINITY, INFINITY, 0.f};
  }
  return TerrainCell{-INFINITY, INFINITY, -INFINITY, INFINITY, 0.f};
}

// floor(x) as an integer in one instruction (saturating, NaN -> 0: no guard needed for rays that miss)
__device__ __forceinline__ int floor_int(float x) {
  int r;
  asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(r) : "v"(x));
  return r;
}

// R * v, row-major R: the rotation of a ray or a cone axis into the world (mat_vec of nmf_device.h under this header's pragma)
__device__ __forceinline__ V3 rot3(const float* R, V3 v) {
  return v3(R[0] * v.x + R[1] * v.y + R[2] * v.z, R[3] * v.x + R[4] * v.y + R[5] * v.z, R[6] * v.x + R[7] * v.y + R[8] * v.z);
}

// a value that is the same in every lane, into a scalar register
__device__ __forceinline__ float uni(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v))); }

// the rgb word of material `mtl` of a kernel's argument struct (a scalar load)
template <class Args>
__device__ __forceinline__ unsigned int rgb_word(const Args& A, int mtl) { unsigned int v; __builtin_memcpy(&v, A.rgb[mtl], 4); return v; }

// the flat ground under the ray cam + t d (hz = cam.z - ground_z, inv_cs = 1 / checker size)
struct GroundHit {
  float t;
  bool hit;
  unsigned int odd;      // checker parity as a mask (bit 0 of the cell sum, sign-extended): ground A xor (mask and (A xor B)) — no select between two scalars
};
__device__ __forceinline__ GroundHit ground_hit(V3 cam, float hz, float inv_cs, V3 d) {
  const float t = -hz * __builtin_amdgcn_rcpf(d.z);
  const float gx = (cam.x + t * d.x) * inv_cs, gy = (cam.y + t * d.y) * inv_cs;
  return GroundHit{t, d.z < 0.f && t > 0.f, (unsigned int)(((floor_int(gx) + floor_int(gy)) << 31) >> 31)};
}

// relief: follow the descending ray (d.z < 0) through the cells of h(x, y) from the highest level down; a cell entered below
// its level is a side wall — wall(t) —, else its top is hit if the ray reaches the level before leaving the cell —
// top(t, odd: the checker parity there).  Neither is called if the ray is still on its way after kMaxTerrainCells cells.
template <class Wall, class Top>
__device__ __forceinline__ void relief_walk(int kind, const float* terrain, float ground_z, V3 cam, float inv_cs, V3 d, Wall&& wall, Top&& top) {
  const float rdz = 1.0f / d.z;
  float tc = fmaxf(0.f, (ground_z + terrain[4] - cam.z) * rdz);
#pragma unroll 1
  for (int it = 0; it < kMaxTerrainCells; ++it) {
    const float tp = tc + kTerrainEps;
    const TerrainCell c = relief_cell(kind, terrain, cam.x + tp * d.x, cam.y + tp * d.y);
    const float h = c.h + ground_z;
    const float z_in = cam.z + tc * d.z;
    if (z_in < h - kTerrainWallTol) { wall(tc); break; }
    const float tx = d.x > 0.f ? (c.x1 - cam.x) / d.x : (d.x < 0.f ? (c.x0 - cam.x) / d.x : INFINITY);
    const float ty = d.y > 0.f ? (c.y1 - cam.y) / d.y : (d.y < 0.f ? (c.y0 - cam.y) / d.y : INFINITY);
    const float t_out = fminf(tx, ty);
    const float t_h = (h - cam.z) * rdz;
    if (t_h <= t_out) {
      const float qx = (cam.x + t_h * d.x) * inv_cs, qy = (cam.y + t_h * d.y) * inv_cs;
      top(t_h, ((floor_int(qx) + floor_int(qy)) & 1) != 0);
      break;
    }
    tc = t_out;
  }
}

}  // namespace nmf
