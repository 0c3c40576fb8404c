// nmf_camera.hip — batch camera renderer for selected worlds of a batch (gfx950): the camera a person looks through.
//
// Replaces the reference's WarpGPUBatchRenderer (warp/rendering.py:279-341: mjw.refit_bvh + mjw.render + a gather of the selected
// worlds and cameras, attached by warp/simulation.py:266-342).  Camera model, scene and shading are build-defined
// and pinned by the numpy specification tests/camera_spec.py: pinhole cameras ("fixed" in the world, or "track": at the fly's
// root segment + a constant offset, orientation constant in the world), the eyes' scene (checker ground or the terrain relief of
// the physics, sky, up to 8 spheres) plus the WHOLE fly as capsules, each with its own colour, lit by one directional light from
// straight above: colour = base * (ambient + diffuse * max(0, n_z)).
//
// Grid: (32 x 32-pixel image tile, camera, selected world) — the world comes from a device list, so 4 of 4096 worlds cost 4
// worlds.  Per workgroup, once: the camera pose and the capsules' world-space end points relative to the camera, in LDS.  A
// wave takes 8 x 8-pixel patches of the tile, one pixel per lane: it culls once per patch, lane = object, against the patch's
// bounding cone (two rounds: capsules 0..63, then capsules 64..71 and the spheres) and decides whether any ray of the patch
// points below the horizon, exactly as the eye kernel does per group; then every lane intersects the survivors only (loops over
// wave-uniform bit masks: scalar control flow), keeps the nearest hit with the z component of its normal, shades and converts.
// The tile is staged in LDS and leaves as dwords of whole row segments.
//
// A world with several flies (one batch per fly, same world ids) is drawn by nmf_camera_flies_kernel: the same tile code with the
// flies in an outer loop.  Ground and spheres come first, once; then one fly at a time is staged in the SAME LDS arrays and every
// patch of the tile is culled and intersected against it; shading comes last.  Between these steps a pixel's nearest hit waits
// in LDS (12 bytes per pixel of the tile: 26.1 KB per workgroup in all).  Carrying the four patches' hits in registers instead
// takes the pass loops unrolled, 107 VGPRs against 72 and 4 waves per SIMD against 6, and measured 15 % slower.
// The hit rule is the one rule of this file — `t < tbest`, strictly — so on an exact tie the earlier object
// wins: ground / terrain, spheres, then capsules in the order (fly, capsule), which is what tests/camera_spec.py does with the
// flies' capsules concatenated.  A fly none of whose capsules' covers meets the tile's bounding cone is left out for the whole
// tile (one workgroup-wide vote after staging it).
//
// Shared with the eye kernel, one definition each in nmf_scene.h: the relief's cells and the walk of a ray through them (this
// file's callbacks also record n_z and `lit`), the flat ground hit and rot3.  The staging of the cover discs and of a capsule's
// end points and the cone-against-disc test (`meets`) are written out in both files; nmf_scene.h says why.  Not shared, on
// purpose: the ray-sphere and ray-capsule intersections, the pinhole, the capd layout and the tile output.  They carry the hit's
// normal, which the eyes do not need, and take their discriminants in a better-conditioned form (see `ball` below: the shade of
// a grazing hit needs it, a material id does not), while the eye frames are pinned pixel for pixel on the textbook form.  This
// file uses nothing that nmf_eyes.hip defines.
#include "nmf_device.h"
#include "nmf_scene.h"

#pragma clang fp reassociate(off)

namespace nmf {

constexpr int kCamThreads = 256;
constexpr int kCamTile = 32;             // a workgroup's tile: 32 x 32 pixels, sixteen 8 x 8 patches, four per wave
constexpr int kCamMaxCaps = 72;          // the engine's segment limit (the eyes see at most 64 of them)
constexpr int kCamMaxFlies = 4;          // flies of one world in one image (NMF_CAMERA_MAX_FLIES)
constexpr int kCamMaxViews = 8;          // cameras per plan (NMF_CAMERA_MAX)

struct CamView {
  int mode, seg;            // 0 fixed: pos is a world position; 1 track: pos is added to the position of segment `seg`
  float pos[3];
  float rot[9];             // camera axes in the world (columns: right, up, back), row-major
  float tan_px;             // tan(fovy / 2) / (H / 2): camera-frame extent of a pixel at unit depth
};

struct CamArgs {
  int height, width, tiles_x;
  float ambient, diffuse;
  float checker_size, ground_z;
  int n_spheres, sphere_stride;
  int terrain_kind;
  float terrain[5];
  int n_caps;
  unsigned char rgb[4 + kMaxSpheres][4];    // 0 sky, 1 ground A, 2 ground B, 3 terrain side wall, 4.. spheres
};

struct CamFly {             // one fly of the scene: the poses of its batch and its capsules
  const float* seg_xpos;
  const float* seg_xquat;
  const int* cap_seg;
  const float* cap_geom;
  const unsigned int* cap_rgb;
  int nseg, n_caps;
};

struct CamFlies {
  CamFly fly[kCamMaxFlies];
  int n_flies;
  int cam_fly[kCamMaxViews];      // the fly a "track" camera follows
};

struct CamHit {             // a pixel's nearest hit so far
  unsigned int rgb;
  float tbest, nz;
  bool lit;                 // the sky has no surface: its colour is not shaded
};

// One tile of one camera's image of one world.  kFlies = false: the scene's one fly G.fly[0], each patch from culling to
// shading in one go.  kFlies = true: G.n_flies flies, one after the other through the same LDS arrays (the file's head).
template <bool kFlies>
__device__ __forceinline__ void camera_tile(const CamArgs& A, const CamView* __restrict__ views, const int* __restrict__ world_ids,
                                            const CamFlies& G, const float* __restrict__ spheres, uint8_t* __restrict__ frames_out) {
  // capsules relative to the camera, world axes: 0-2 pa, 3-5 unit axis n, 6 length, 7 -pa.n, 8-10 the part of -pa across the axis,
  // 11 r^2, 12 1 / r, 13-15 pb, 16 the colour word
  __shared__ float capd[kCamMaxCaps][20];
  __shared__ float capc[kCamMaxCaps][3][5];      // angular cover: three discs (unit direction, cos / sin of the angular radius)
  __shared__ float sph[kMaxSpheres][8];          // centre - camera, r^2, 1 / r, the colour word
  __shared__ float sphc[kMaxSpheres][5];
  __shared__ float camp[3];
  __shared__ unsigned int tile[kCamTile * kCamTile * 3 / 4];

  const int cam_i = blockIdx.y, sel = blockIdx.z;
  const int w = world_ids[sel];
  const CamView& V = views[cam_i];
  if (threadIdx.x < 3) {
    float p = V.pos[threadIdx.x];
    if (V.mode == 1) {
      const CamFly& T = G.fly[kFlies ? G.cam_fly[cam_i] : 0];
      p += T.seg_xpos[((size_t)w * T.nseg + V.seg) * 3 + threadIdx.x];
    }
    camp[threadIdx.x] = p;
  }
  __syncthreads();
  const V3 cam = v3(uni(camp[0]), uni(camp[1]), uni(camp[2]));
  float R[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = uni(V.rot[i]);
  const float tpx = uni(V.tan_px);
  if (threadIdx.x < A.n_spheres) {
    const int s = threadIdx.x;
    const float* g = spheres + (size_t)w * A.sphere_stride + 4 * s;
    const float r = g[3];
    const V3 oc = cam - v3(g[0], g[1], g[2]);
    float* q = sph[s];
    q[0] = -oc.x; q[1] = -oc.y; q[2] = -oc.z; q[3] = r * r; q[4] = 1.0f / r;      // centre - camera
    q[5] = __builtin_bit_cast(float, rgb_word(A, 4 + s));
    const float dist = sqrtf(dot(oc, oc));
    const float inv = dist > 1e-6f ? 1.0f / dist : 0.f;
    float* c = sphc[s];
    c[0] = -oc.x * inv; c[1] = -oc.y * inv; c[2] = -oc.z * inv;
    const float ang = dist > r ? asinf(r / dist) + 0.03f : 3.2f;
    c[3] = ang < 3.1f ? cosf(ang) : -2.f; c[4] = ang < 3.1f ? sinf(ang) : 0.f;
  }
  // a fly's capsules into capd / capc: lane = capsule
  auto stage = [&](const CamFly& F) {
    if (threadIdx.x >= 64 && threadIdx.x - 64 < F.n_caps) {      // (waves 1 and 2: the spheres are wave 0's)
      const int c = threadIdx.x - 64, cs = F.cap_seg[c];
      const float* g = F.cap_geom + 7 * c;
      float Rc[9];
      qmat(Rc, ldq(F.seg_xquat + ((size_t)w * F.nseg + cs) * 4));
      const V3 xp = ld3(F.seg_xpos + ((size_t)w * F.nseg + cs) * 3);
      const V3 pa = (xp + mat_vec(Rc, ld3(g))) - cam, pb = (xp + mat_vec(Rc, ld3(g + 3))) - cam;
      const float r = g[6];
      const V3 ba = pb - pa;
      const float baba = dot(ba, ba);
      const float len = sqrtf(baba), ilen = len > 1e-9f ? 1.0f / len : 0.f;
      const V3 nx = ilen * ba;
      const float on = -dot(pa, nx);
      float* q = capd[c];
      q[0] = pa.x; q[1] = pa.y; q[2] = pa.z; q[3] = nx.x; q[4] = nx.y; q[5] = nx.z; q[6] = len; q[7] = on;
      q[8] = -pa.x - on * nx.x; q[9] = -pa.y - on * nx.y; q[10] = -pa.z - on * nx.z;
      q[11] = r * r; q[12] = 1.0f / r; q[13] = pb.x; q[14] = pb.y; q[15] = pb.z;
      q[16] = __builtin_bit_cast(float, F.cap_rgb[c]); q[17] = 0.f; q[18] = 0.f; q[19] = 0.f;
      // angular cover as in the eye kernel: the thirds of the axis, each inside a sphere of radius (length / 6 + r)
      const float Rb = sqrtf(baba) * (1.0f / 6.0f) + r;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const V3 mid = pa + ((2.f * (float)i + 1.f) * (1.0f / 6.0f)) * ba;
        const float dist = sqrtf(dot(mid, mid));
        const float inv = dist > 1e-6f ? 1.0f / dist : 0.f;
        const float ang = dist > Rb ? asinf(Rb / dist) + 0.004f : 3.2f;       // camera inside the bound: always a candidate
        float* cq = capc[c][i];
        cq[0] = mid.x * inv; cq[1] = mid.y * inv; cq[2] = mid.z * inv;
        cq[3] = ang < 3.1f ? cosf(ang) : -2.f; cq[4] = ang < 3.1f ? sinf(ang) : 0.f;
      }
    }
  };
  if constexpr (!kFlies) stage(G.fly[0]);
  __syncthreads();

  const unsigned int w_sky = rgb_word(A, 0), w_ga = rgb_word(A, 1), w_gb = rgb_word(A, 2), w_wall = rgb_word(A, 3), w_gx = w_ga ^ w_gb;
  const float inv_cs = 1.0f / A.checker_size;
  const float hz = cam.z - A.ground_z;
  const float cx = 0.5f * (float)A.width, cy = 0.5f * (float)A.height;
  const int tile_y = blockIdx.x / A.tiles_x, tile_x = blockIdx.x - tile_y * A.tiles_x;
  const int row0 = tile_y * kCamTile, col0 = tile_x * kCamTile;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lx = lane & 7, ly = lane >> 3;
  uint8_t* const tile_b = reinterpret_cast<uint8_t*>(tile);

  // does a cone (axis a, half-angle by cos / sin) meet a disc of angular radius (qc, qs) about the unit direction q?  (nmf_eyes.hip)
  auto meets = [](V3 a, float c_cos, float c_sin, const float* q) {
    const float ca = q[0] * a.x + q[1] * a.y + q[2] * a.z;
    return (int)(q[3] < -1.5f) | (int)(ca >= c_cos * q[3] - c_sin * q[4]) | (int)(c_sin * q[3] + c_cos * q[4] <= 0.f);
  };
  // bounding cone of the rays of the pixels [pr0, pr0 + 2 half) x [pc0, pc0 + 2 half): the axis through the centre (world frame:
  // gw), the widest of the four corners; g_raw: the cosine before the margin and the clamp
  auto cone = [&](int pr0, int pc0, int half, V3& gw, float& g_cos, float& g_sin, float& g_raw) {
    const float uc = ((float)(pc0 + half) - cx) * tpx, vc = ((float)(pr0 + half) - cy) * tpx;
    const float ic = __builtin_amdgcn_rsqf(uc * uc + vc * vc + 1.f);
    const V3 ax_c = v3(uc * ic, -vc * ic, -ic);
    g_cos = 1.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float u = ((float)(pc0 + 2 * half * (k & 1)) - cx) * tpx, v = ((float)(pr0 + 2 * half * (k >> 1)) - cy) * tpx;
      const float in = __builtin_amdgcn_rsqf(u * u + v * v + 1.f);
      g_cos = fminf(g_cos, (u * ax_c.x - v * ax_c.y - ax_c.z) * in);
    }
    g_raw = g_cos;
    g_cos = fmaxf(g_cos - 1e-5f, 0.f);       // (a patch of a pinhole image spans far less than a right angle)
    g_sin = sqrtf(fmaxf(1.f - g_cos * g_cos, 0.f));
    gw = rot3(R, ax_c);
  };
  // culling, lane = object.  Round 1: capsules 0..63; round 2: lanes 0..7 = capsules 64..71, lanes 8..15 = the spheres
  auto cull_lo = [&](V3 gw, float g_cos, float g_sin, int n_caps) {
    int sees = 0;
    if (lane < n_caps) {
#pragma unroll
      for (int i = 0; i < 3; ++i) sees |= meets(gw, g_cos, g_sin, capc[lane][i]);
    }
    return __ballot(sees != 0);
  };
  auto cull_hi = [&](V3 gw, float g_cos, float g_sin, int n_caps, int n_spheres) {
    int sees = 0;
    if (lane < 8 && 64 + lane < n_caps) {
#pragma unroll
      for (int i = 0; i < 3; ++i) sees |= meets(gw, g_cos, g_sin, capc[64 + lane][i]);
    } else if (lane >= 8 && lane < 8 + n_spheres) {
      sees = meets(gw, g_cos, g_sin, sphc[lane - 8]);
    }
    return (unsigned int)__ballot(sees != 0);
  };
  // this lane's ray through the pixel (row, col)
  auto ray = [&](int row, int col) {
    const float u = ((float)col + 0.5f - cx) * tpx, v = ((float)row + 0.5f - cy) * tpx;
    const float inorm = __builtin_amdgcn_rsqf(u * u + v * v + 1.f);
    return rot3(R, v3(u * inorm, -v * inorm, -inorm));
  };
  // Discriminants in the well-conditioned form: a ray (unit d) passes a point c at the distance |d x c|, so it meets the sphere
  // of radius r about c iff r^2 - |d x c|^2 >= 0 — a difference of two numbers of the size of r^2.  The textbook form
  // (d.c)^2 - (c.c - r^2) subtracts numbers of the size of the DISTANCE squared: with a 0.1 mm leg segment 10 mm away float32
  // loses four digits there, the root moves by micrometres along a grazing ray and the normal — hence the shade — by several
  // grey levels at every silhouette.
  auto ball = [](const V3& d, float cx_, float cy_, float cz_, float r2, float& t) {       // nearest hit with the sphere about c; false: the ray misses it
    const float kx = d.y * cz_ - d.z * cy_, ky = d.z * cx_ - d.x * cz_, kz = d.x * cy_ - d.y * cx_;
    const float disc = r2 - (kx * kx + ky * ky + kz * kz);
    t = (d.x * cx_ + d.y * cy_ + d.z * cz_) - __builtin_amdgcn_sqrtf(fmaxf(disc, 0.f));
    return disc > 0.f && t > 0.f;
  };
  // sky, ground or relief, and the spheres of the mask
  auto scene = [&](const V3& d, bool grp_ground, unsigned int grp_sph) {
    CamHit h{w_sky, INFINITY, 0.f, false};
    if (grp_ground) {
      const GroundHit g = ground_hit(cam, hz, inv_cs, d);
      h.rgb = g.hit ? (w_ga ^ (g.odd & w_gx)) : w_sky;
      h.tbest = g.hit ? g.t : INFINITY; h.nz = 1.f; h.lit = g.hit;
      // the relief instead, where the world has one: a top has n_z = 1, a side wall n_z = 0
      if (A.terrain_kind != 0 && d.z < 0.f)
        relief_walk(A.terrain_kind, A.terrain, A.ground_z, cam, inv_cs, d,
                    [&](float t) { h.tbest = t; h.rgb = w_wall; h.nz = 0.f; h.lit = true; },
                    [&](float t, bool odd) { h.tbest = t; h.rgb = odd ? w_gb : w_ga; h.nz = 1.f; h.lit = true; });
    }
    for (unsigned int sm = grp_sph; sm; sm &= sm - 1u) {
      const int s = __ffs((int)sm) - 1;
      const float* q = sph[s];
      float ts;
      const bool ok = ball(d, q[0], q[1], q[2], q[3], ts) && ts < h.tbest;
      if (ok) { h.tbest = ts; h.rgb = __builtin_bit_cast(unsigned int, q[5]); h.nz = (ts * d.z - q[2]) * q[4]; h.lit = true; }
    }
    return h;
  };
  auto capsule = [&](const V3& d, CamHit& h, int ci) {
    const float* q = capd[ci];
    // across the axis n: the ray's direction dp and the camera's offset op (from the capsule's data); the side is hit where
    // the ray passes the axis at the distance r: a t^2 + 2 (dp.op) t + |op|^2 - r^2 = 0, discriminant a r^2 - |dp x op|^2
    const float dn = q[3] * d.x + q[4] * d.y + q[5] * d.z;
    const float px = d.x - dn * q[3], py = d.y - dn * q[4], pz = d.z - dn * q[5];
    const float a = px * px + py * py + pz * pz;
    const float kx = py * q[10] - pz * q[9], ky = pz * q[8] - px * q[10], kz = px * q[9] - py * q[8];
    const float hq = a * q[11] - (kx * kx + ky * ky + kz * kz);
    const float tb = (-(px * q[8] + py * q[9] + pz * q[10]) - __builtin_amdgcn_sqrtf(fmaxf(hq, 0.f))) / a;
    const float yy = q[7] + tb * dn;             // along the axis, from pa
    const bool cyl = hq >= 0.f && a > 1e-12f;
    float tcap = INFINITY, zc = 0.f;        // zc: z of the axis point the hit's normal starts from (relative to the camera)
    if (cyl && yy > 0.f && yy < q[6] && tb > 0.f) { tcap = tb; zc = q[2] + q[5] * yy; }
    else {
      const bool use_a = !(yy > 0.f) || !cyl;
      float te;
      const bool hit_end = ball(d, use_a ? q[0] : q[13], use_a ? q[1] : q[14], use_a ? q[2] : q[15], q[11], te);
      if (hit_end) { tcap = te; zc = use_a ? q[2] : q[15]; }
    }
    if (tcap < h.tbest) { h.tbest = tcap; h.rgb = __builtin_bit_cast(unsigned int, q[16]); h.nz = (tcap * d.z - zc) * q[12]; h.lit = true; }
  };
  auto capsules = [&](const V3& d, CamHit& h, unsigned long long caps_lo, unsigned int caps_hi) {
    for (unsigned long long cm = caps_lo; cm; cm &= cm - 1ull) capsule(d, h, __ffsll((long long)cm) - 1);
    for (unsigned int cm = caps_hi; cm; cm &= cm - 1u) capsule(d, h, 64 + __ffs((int)cm) - 1);
  };
  // one light from straight above; rounded as vision._u8 rounds (floor(x + 0.5)), saturating
  auto shade = [&](int pass, const CamHit& h) {
    const float f = h.lit ? A.ambient + A.diffuse * fmaxf(h.nz, 0.f) : 1.f;
    uint8_t* o = tile_b + ((8 * pass + ly) * kCamTile + 8 * wave + lx) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float x = (float)((h.rgb >> (8 * c)) & 0xffu) * f + 0.5f;
      o[c] = (uint8_t)min(max(floor_int(x), 0), 255);
    }
  };

  // the wave's patch of a pass: 8 x 8 pixels at (row0 + 8 pass, col0 + 8 wave); wholly outside the image (wave-uniform): no work
  const int pc0 = col0 + 8 * wave;
  if constexpr (!kFlies) {
#pragma unroll 1
    for (int pass = 0; pass < 4; ++pass) {
      const int pr0 = row0 + 8 * pass;
      if (pr0 >= A.height || pc0 >= A.width) continue;
      V3 gw; float g_cos, g_sin, g_raw;
      cone(pr0, pc0, 4, gw, g_cos, g_sin, g_raw);
      const unsigned long long caps_lo = cull_lo(gw, g_cos, g_sin, A.n_caps);
      const unsigned int round2 = cull_hi(gw, g_cos, g_sin, A.n_caps, A.n_spheres);
      const unsigned int caps_hi = round2 & 0xffu, grp_sph = (round2 >> 8) & 0xffu;
      const bool grp_ground = gw.z < g_sin + 1e-3f;                // some ray of the patch points below the horizon
      const V3 d = ray(pr0 + ly, pc0 + lx);
      CamHit h = scene(d, grp_ground, grp_sph);
      capsules(d, h, caps_lo, caps_hi);
      shade(pass, h);
    }
  } else {
    // the tile's own bounding cone, for the vote on a whole fly.  A cone that nears a right angle (a huge field of view on a
    // tiny image) is past the clamp's premise: then every fly is a candidate
    V3 tw; float t_cos, t_sin, t_raw;
    cone(row0, col0, kCamTile / 2, tw, t_cos, t_sin, t_raw);
    auto stage_and_vote = [&](const CamFly& F) {
      stage(F);
      int sees = t_raw < 0.25f;
      if (threadIdx.x >= 64 && threadIdx.x - 64 < F.n_caps) {
#pragma unroll
        for (int i = 0; i < 3; ++i) sees |= meets(tw, t_cos, t_sin, capc[threadIdx.x - 64][i]);
      }
      return sees;
    };
    // the first fly is staged ahead of the ground and the spheres: waves 0 and 3 start on those while waves 1 and 2 stage
    int sees = stage_and_vote(G.fly[0]);
    // a pixel's nearest hit between the steps: each thread reads and writes its own slots only (`lit` rides in the colour word's
    // unused byte)
    __shared__ float hit_t[4][kCamThreads], hit_nz[4][kCamThreads];
    __shared__ unsigned int hit_rgb[4][kCamThreads];
    auto put = [&](int pass, const CamHit& h) {
      hit_t[pass][threadIdx.x] = h.tbest; hit_nz[pass][threadIdx.x] = h.nz; hit_rgb[pass][threadIdx.x] = h.rgb | (h.lit ? 1u << 24 : 0u);
    };
    auto get = [&](int pass) {
      const unsigned int v = hit_rgb[pass][threadIdx.x];
      return CamHit{v & 0xffffffu, hit_t[pass][threadIdx.x], hit_nz[pass][threadIdx.x], (v >> 24) != 0};
    };
#pragma unroll 1
    for (int pass = 0; pass < 4; ++pass) {
      const int pr0 = row0 + 8 * pass;
      if (pr0 < A.height && pc0 < A.width) {
        V3 gw; float g_cos, g_sin, g_raw;
        cone(pr0, pc0, 4, gw, g_cos, g_sin, g_raw);
        const unsigned int grp_sph = (cull_hi(gw, g_cos, g_sin, 0, A.n_spheres) >> 8) & 0xffu;
        put(pass, scene(ray(pr0 + ly, pc0 + lx), gw.z < g_sin + 1e-3f, grp_sph));
      }
    }
#pragma unroll 1
    for (int f = 0; f < G.n_flies; ++f) {
      const CamFly& F = G.fly[f];
      if (f > 0) {
        __syncthreads();                     // every wave is done with the fly before
        sees = stage_and_vote(F);
      }
      if (!__syncthreads_or(sees)) continue;       // (the same answer in every thread of the workgroup; the fly is staged)
#pragma unroll 1
      for (int pass = 0; pass < 4; ++pass) {
        const int pr0 = row0 + 8 * pass;
        if (pr0 < A.height && pc0 < A.width) {
          V3 gw; float g_cos, g_sin, g_raw;
          cone(pr0, pc0, 4, gw, g_cos, g_sin, g_raw);
          const unsigned long long caps_lo = cull_lo(gw, g_cos, g_sin, F.n_caps);
          const unsigned int caps_hi = cull_hi(gw, g_cos, g_sin, F.n_caps, 0) & 0xffu;
          if (caps_lo | caps_hi) { CamHit h = get(pass); capsules(ray(pr0 + ly, pc0 + lx), h, caps_lo, caps_hi); put(pass, h); }
        }
      }
    }
#pragma unroll 1
    for (int pass = 0; pass < 4; ++pass)
      if (row0 + 8 * pass < A.height && pc0 < A.width) shade(pass, get(pass));
  }
  __syncthreads();

  // the tile leaves as dwords of whole row segments: a row of the tile is [g0, g1) of the frame array's bytes; its aligned
  // dwords are assembled from the staged bytes, the (at most 3 + 3) bytes before and after them — only where the row segment
  // does not start or end on a dword: image widths that are no multiple of 4 — go out as bytes
  const int wseg = min(kCamTile, A.width - col0), hseg = min(kCamTile, A.height - row0);
  const size_t frame0 = ((size_t)sel * gridDim.y + cam_i) * (size_t)A.height * A.width * 3;
  for (int i = threadIdx.x; i < hseg * 24; i += kCamThreads) {
    const int r = i / 24, k = i - r * 24;
    const size_t g0 = frame0 + ((size_t)(row0 + r) * A.width + col0) * 3, g1 = g0 + (size_t)wseg * 3;
    const size_t a0 = (g0 + 3) & ~(size_t)3;
    const size_t a = a0 + 4 * (size_t)k;
    const uint8_t* src = tile_b + r * kCamTile * 3;
    if (a + 4 <= g1) {
      const int off = (int)(a - g0);
      const unsigned int word = (unsigned int)src[off] | ((unsigned int)src[off + 1] << 8) | ((unsigned int)src[off + 2] << 16) | ((unsigned int)src[off + 3] << 24);
      *reinterpret_cast<unsigned int*>(frames_out + a) = word;
    }
    if (k == 0) {
      for (size_t p = g0; p < a0 && p < g1; ++p) frames_out[p] = src[p - g0];
      const size_t tail = a0 + ((g1 > a0 ? g1 - a0 : 0) & ~(size_t)3);
      for (size_t p = tail > g0 ? tail : g0; p < g1; ++p) if (p >= a0) frames_out[p] = src[p - g0];
    }
  }
}

__global__ void __launch_bounds__(kCamThreads)
nmf_camera_kernel(CamArgs A, const CamView* __restrict__ views, const int* __restrict__ world_ids,
                  const float* __restrict__ seg_xpos, const float* __restrict__ seg_xquat, int nseg,
                  const float* __restrict__ spheres, const int* __restrict__ cap_seg, const float* __restrict__ cap_geom,
                  const unsigned int* __restrict__ cap_rgb, uint8_t* __restrict__ frames_out) {
  CamFlies G;
  G.fly[0] = CamFly{seg_xpos, seg_xquat, cap_seg, cap_geom, cap_rgb, nseg, A.n_caps};
  G.n_flies = 1;
  camera_tile<false>(A, views, world_ids, G, spheres, frames_out);
}

// A.n_caps is not read: each fly has its own count
__global__ void __launch_bounds__(kCamThreads)
nmf_camera_flies_kernel(CamArgs A, CamFlies G, const CamView* __restrict__ views, const int* __restrict__ world_ids,
                        const float* __restrict__ spheres, uint8_t* __restrict__ frames_out) {
  camera_tile<true>(A, views, world_ids, G, spheres, frames_out);
}

}  // namespace nmf
