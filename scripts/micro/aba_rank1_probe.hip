// checks what the leg-chain kernels' articulated-body sweeps (nmf_step_aba.h) rely on since their rank-1 downdates run on the
// matrix pipe: grp8_rank1_mfma (nmf_device.h) — row r of a 6 x 6 matrix in lane r of an 8-lane group, rows 6 and 7 shadows —
// leaves in every lane, shadow lanes included, bit for bit
//   IA[c] = fmaf(nk of the lane, U of the group's lane c, IA[c]),  c = 0 .. 5,
// through chains of 17 successive downdates (the length of a sweep's chain).  Four forms of the chain on the GPU:
//   the one it replaces (six ds_swizzle broadcasts + three v_pk_fma_f32: grp8_bcast, fma6),
//   the matrix instruction with its own A broadcast (CBSZ = 1, ABID = 0 / 1),
//   the matrix instruction fed by the two DPP copies (grp8_lo, grp8_hi),
//   the broadcast form once more with the pad registers CARRIED along the chain from a NaN,
// compared word by word on the GPU; the first matrix form also against fmaf on the host.  Shadow lanes' U feeds the pad columns
// only: in half of the groups it is a NaN, which must not show anywhere.  The lane maps of grp8_lo, grp8_hi and grp8_bcast_dpp
// are checked on lane numbers.  Inputs (a counter hash, the same on both sides): full mantissas whose products need more than
// 24 bits, wide exponents (products underflow to subnormals and to zero), zeros of both signs and subnormals, short mantissas
// with the half-ulp bit (ties).  Prints the counts; exit status 0 only if every word agrees.
#include <hip/hip_runtime.h>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "nmf_device.h"

constexpr int kSteps = 17, kWaves = 131072, kGroups = kWaves * 8;      // 1 048 576 groups of eight lanes

__host__ __device__ inline uint32_t mix(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}
// input number `slot` of lane `r` of group `g` as a bit pattern
__host__ __device__ inline uint32_t sample_bits(uint32_t g, uint32_t r, uint32_t slot) {
  const uint32_t h = mix(mix(g * 0x9e3779b9u + 0x85ebca6bu) ^ (slot * 8u + r) * 0xc2b2ae35u), h2 = mix(h + 0x27d4eb2fu);
  const uint32_t mant = h & 0x7fffffu, sign = h2 & 0x80000000u, e = (h2 >> 8) & 0xffffu, pick = h2 & 7u;
  switch (g & 3u) {
    case 0: return sign | ((120u + e % 14u) << 23) | mant;                                  // 2^-7 .. 2^6, full mantissas
    case 1: return sign | ((34u + e % 127u) << 23) | mant;                                  // 2^-93 .. 2^33: products underflow
    case 2: return pick == 0 ? sign : pick == 1 ? (sign | mant) /* subnormal */ : (sign | ((100u + e % 40u) << 23) | mant);
    default: return sign | (127u << 23) | (mant & 0x7ff000u) | 0x800u;                       // ties
  }
}
// slots: 0 .. 5 the lane's row, then per step U and nk.  Shadow lanes' U: a NaN in the groups with bit 2 set.
__host__ __device__ inline uint32_t u_bits(uint32_t g, uint32_t r, int t) { return r >= 6 && (g & 4u) ? 0x7fc00000u : sample_bits(g, r, 6 + 2 * t); }
__host__ __device__ inline uint32_t nk_bits(uint32_t g, uint32_t r, int t) { return sample_bits(g, r, 7 + 2 * t); }

__device__ __forceinline__ float f_of(uint32_t u) { return __builtin_bit_cast(float, u); }
__device__ __forceinline__ uint32_t u_of(float f) { return __builtin_bit_cast(uint32_t, f); }

// out[group][lane of the group][6]: the broadcast form's result.  bad[0..2]: words of the other three forms that differ from it.
__global__ void __launch_bounds__(64) probe(uint32_t* out, unsigned int* bad) {
  using namespace nmf;
  const int lane = threadIdx.x;
  const uint32_t g = blockIdx.x * 8u + (lane >> 3), r = lane & 7;
  float a[6], b[6], c[6], d[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) a[i] = b[i] = c[i] = d[i] = f_of(sample_bits(g, r, i));
  float pad2 = f_of(0x7fc00000u), pad3 = pad2;
#pragma unroll
  for (int t = 0; t < kSteps; ++t) {
    const float U = f_of(u_bits(g, r, t)), nk = f_of(nk_bits(g, r, t));
    { const float bb[6] = {grp8_bcast<0>(U), grp8_bcast<1>(U), grp8_bcast<2>(U), grp8_bcast<3>(U), grp8_bcast<4>(U), grp8_bcast<5>(U)};
      fma6(a, nk, bb); }
    grp8_rank1_mfma<false>(b, nk, U);
    grp8_rank1_mfma<true>(c, nk, U);
    { f32x4 lo = {d[0], d[1], d[2], d[3]}, hi = {d[4], d[5], pad2, pad3};
      lo = __builtin_amdgcn_mfma_f32_4x4x1f32(U, nk, lo, 1, 0, 0);
      hi = __builtin_amdgcn_mfma_f32_4x4x1f32(U, nk, hi, 1, 1, 0);
      d[0] = lo[0]; d[1] = lo[1]; d[2] = lo[2]; d[3] = lo[3]; d[4] = hi[0]; d[5] = hi[1]; pad2 = hi[2]; pad3 = hi[3]; }
  }
  unsigned int na = 0, nc = 0, nd = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    out[((size_t)g * 8 + r) * 6 + i] = u_of(b[i]);
    na += u_of(a[i]) != u_of(b[i]); nc += u_of(c[i]) != u_of(b[i]); nd += u_of(d[i]) != u_of(b[i]);
  }
  if (na) atomicAdd(&bad[0], na);
  if (nc) atomicAdd(&bad[1], nc);
  if (nd) atomicAdd(&bad[2], nd);
}

// maps[k][lane]: the lane a value comes from under grp8_lo (k = 0), grp8_hi (1), grp8_bcast_dpp<0..7> (2..9), grp8_bcast<0..7> (10..17)
__global__ void __launch_bounds__(64) lane_maps(float* maps) {
  using namespace nmf;
  const int lane = threadIdx.x;
  const float v = (float)lane;
  maps[lane] = grp8_lo(v);
  maps[64 + lane] = grp8_hi(v);
  static_for<8>([&](auto I) {
    constexpr int i = decltype(I)::value;
    maps[(2 + i) * 64 + lane] = grp8_bcast_dpp<i>(v);
    maps[(10 + i) * 64 + lane] = grp8_bcast<i>(v);
  });
}

static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

int main() {
  const size_t nout = (size_t)kGroups * 48;
  const auto t0 = std::chrono::steady_clock::now();
  auto since = [&] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };
  uint32_t* dout; unsigned int* dbad; float* dmaps;
  HIP_OK(hipMalloc(&dout, nout * 4)); HIP_OK(hipMalloc(&dbad, 3 * 4)); HIP_OK(hipMalloc(&dmaps, 18 * 64 * 4));
  HIP_OK(hipMemset(dout, 0xff, nout * 4)); HIP_OK(hipMemset(dbad, 0, 3 * 4)); HIP_OK(hipMemset(dmaps, 0xff, 18 * 64 * 4));
  lane_maps<<<1, 64>>>(dmaps);
  probe<<<kWaves, 64>>>(dout, dbad);
  HIP_OK(hipGetLastError()); HIP_OK(hipDeviceSynchronize());
  std::vector<uint32_t> out(nout); unsigned int bad[3]; float maps[18 * 64];
  HIP_OK(hipMemcpy(out.data(), dout, nout * 4, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(bad, dbad, sizeof bad, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(maps, dmaps, sizeof maps, hipMemcpyDeviceToHost));
  const double t_gpu = since();

  long bad_map = 0;
  for (int lane = 0; lane < 64; ++lane) {
    const int g8 = lane & ~7, r = lane & 7;
    bad_map += maps[lane] != (float)(g8 + (r & 3));
    bad_map += maps[64 + lane] != (float)(g8 + 4 + (r & 3));
    for (int i = 0; i < 8; ++i) { bad_map += maps[(2 + i) * 64 + lane] != (float)(g8 + i); bad_map += maps[(10 + i) * 64 + lane] != (float)(g8 + i); }
  }
  if (bad_map) {
    printf("grp8_lo  :"); for (int l = 0; l < 16; ++l) printf(" %g", maps[l]); printf("\n");
    printf("grp8_hi  :"); for (int l = 0; l < 16; ++l) printf(" %g", maps[64 + l]); printf("\n");
  }

  // the host's chain, on a few threads (816 million fmaf; the products that need the extra bits are counted in every 16th group)
  constexpr int kThreads = 16;
  long bad_host[kThreads] = {}, inexact[kThreads] = {}, subn[kThreads] = {}, zeros[kThreads] = {}, nans[kThreads] = {};
  std::vector<std::thread> pool;
  for (int th = 0; th < kThreads; ++th)
    pool.emplace_back([&, th] {
      long n_bad = 0, n_inexact = 0, n_subn = 0, n_zeros = 0, n_nans = 0;      // (own counters: the arrays' slots share cache lines)
      for (uint32_t g = th; g < (uint32_t)kGroups; g += kThreads) {
        float U[kSteps][8];
        for (int t = 0; t < kSteps; ++t)
          for (uint32_t r = 0; r < 8; ++r) U[t][r] = from_bits(u_bits(g, r, t));
        for (uint32_t r = 0; r < 8; ++r) {
          float ia[6];
          for (int i = 0; i < 6; ++i) ia[i] = from_bits(sample_bits(g, r, i));
          for (int t = 0; t < kSteps; ++t) {
            const float nk = from_bits(nk_bits(g, r, t));
            for (int i = 0; i < 6; ++i) {
              if ((g & 0xf0u) == 0) n_inexact += (double)nk * (double)U[t][i] != (double)(nk * U[t][i]);
              ia[i] = fmaf(nk, U[t][i], ia[i]);
              n_subn += ia[i] != 0.f && std::fabs(ia[i]) < 1.17549435e-38f;
            }
          }
          for (int i = 0; i < 6; ++i) {
            const uint32_t got = out[((size_t)g * 8 + r) * 6 + i];
            n_zeros += ia[i] == 0.f;
            n_nans += std::isnan(from_bits(got));
            if (got != bits(ia[i])) {
              if (n_bad++ < 2) printf("group %u lane %u column %d: mfma %08x host %08x\n", g, r, i, got, bits(ia[i]));
            }
          }
        }
      }
      bad_host[th] = n_bad; inexact[th] = n_inexact; subn[th] = n_subn; zeros[th] = n_zeros; nans[th] = n_nans;
    });
  for (auto& t : pool) t.join();
  long bh = 0, ix = 0, sb = 0, zr = 0, nn = 0;
  for (int th = 0; th < kThreads; ++th) { bh += bad_host[th]; ix += inexact[th]; sb += subn[th]; zr += zeros[th]; nn += nans[th]; }
  printf("aba_rank1_probe: %d groups of eight lanes, chains of %d downdates, %zu result words (%ld of the %ld products looked at need the extra bits; "
         "%ld subnormal intermediate results, %ld zero results, %ld NaN results); GPU part %.1f s, host part %.1f s\n",
         kGroups, kSteps, nout, ix, (long)kGroups / 16 * 8 * kSteps * 6, sb, zr, nn, t_gpu, since() - t_gpu);
  printf("  lane maps of grp8_lo, grp8_hi, grp8_bcast_dpp, grp8_bcast: %ld differ\n", bad_map);
  printf("  mfma (A broadcast) vs host fmaf chain: %ld differ\n", bh);
  printf("  mfma (A broadcast) vs swizzle + v_pk_fma_f32 on the GPU: %u differ\n", bad[0]);
  printf("  mfma (A broadcast) vs mfma (DPP copies): %u differ\n", bad[1]);
  printf("  mfma (A broadcast) vs the same with pads carried from a NaN: %u differ\n", bad[2]);
  const bool ok = bad_map == 0 && bh == 0 && bad[0] == 0 && bad[1] == 0 && bad[2] == 0 && nn == 0;
  printf(ok ? "PASS: every lane holds fmaf(nk, U of lane c, IA[c]); the pad columns reach no result\n" : "FAIL\n");
  return ok ? 0 : 1;
}
