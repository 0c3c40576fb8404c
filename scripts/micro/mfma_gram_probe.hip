// checks what the Gram block of dual_solve (nmf_dual.h) relies on: v_mfma_f32_4x4x1_16B_f32, sixteen 4 x 4 outer products per
// wave (block = four consecutive lanes), fed one term at a time, is bit for bit the chain
//   acc = +0;  acc = fmaf(a_i, b_i, acc), i = 0 .. 16        (one rounding per multiply-add)
// that the vector pipe computes, and lane 4 q + j, result register i holds (A of lane 4 q + i) x (B of lane 4 q + j).
// (The first term, fma(a, b, +0), is the rounded product a b except that a product of -0 comes out as +0.)
// Three references: the same chain by v_fma_f32 on the GPU, the same chain by fmaf on the host, and the map by a scalar
// triple loop (quad, row, column).  Inputs: random f32 whose products need the extra bits, wide exponents, zeros of both
// signs, subnormals and products that underflow.  Prints the counts; exit status 0 only if every bit agrees.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

constexpr int kTerms = 17, kWave = 64, kCases = 4096;
typedef float f32x4 __attribute__((ext_vector_type(4)));

// a[case][term][lane], b likewise; out_*[case][reg][lane]
__global__ void probe(const float* a, const float* b, float* out_mfma, float* out_valu, int ncases) {
  const int lane = threadIdx.x;
  for (int cs = blockIdx.x; cs < ncases; cs += gridDim.x) {
    const float* A = a + (size_t)cs * kTerms * kWave;
    const float* B = b + (size_t)cs * kTerms * kWave;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < kTerms; ++i) acc = __builtin_amdgcn_mfma_f32_4x4x1f32(A[i * kWave + lane], B[i * kWave + lane], acc, 0, 0, 0);
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int src = (lane & ~3) + r;
      float c = __builtin_fmaf(A[src], B[lane], 0.f);
#pragma unroll
      for (int i = 1; i < kTerms; ++i) c = __builtin_fmaf(A[i * kWave + src], B[i * kWave + lane], c);
      v[r] = c;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      out_mfma[((size_t)cs * 4 + r) * kWave + lane] = acc[r];
      out_valu[((size_t)cs * 4 + r) * kWave + lane] = v[r];
    }
  }
}

static uint32_t rng_state = 0x9e3779b9u;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }
static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float sample(int kind) {
  const uint32_t mant = rnd() & 0x7fffffu, sign = rnd() & 0x80000000u;
  switch (kind) {
    case 0: return from_bits(sign | ((120u + rnd() % 14u) << 23) | mant);          // 2^-7 .. 2^6, full mantissas
    case 1: return from_bits(sign | ((34u + rnd() % 127u) << 23) | mant);          // 2^-93 .. 2^33: products underflow to subnormals and to zero
    case 2: { const uint32_t r = rnd() % 8u; return r == 0 ? from_bits(sign) : r == 1 ? from_bits(sign | mant) /* subnormal */ : from_bits(sign | ((100u + rnd() % 40u) << 23) | mant); }
    default: return from_bits(sign | (127u << 23) | (mant & 0x7ff000u) | 0x800u);   // short mantissas with the half-ulp bit: ties
  }
}

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

int main() {
  const size_t nin = (size_t)kCases * kTerms * kWave, nout = (size_t)kCases * 4 * kWave;
  std::vector<float> a(nin), b(nin), om(nout), ov(nout);
  for (int cs = 0; cs < kCases; ++cs)
    for (int i = 0; i < kTerms * kWave; ++i) { a[(size_t)cs * kTerms * kWave + i] = sample(cs & 3); b[(size_t)cs * kTerms * kWave + i] = sample(cs & 3); }
  float *da, *db, *dm, *dv;
  HIP_OK(hipMalloc(&da, nin * 4)); HIP_OK(hipMalloc(&db, nin * 4)); HIP_OK(hipMalloc(&dm, nout * 4)); HIP_OK(hipMalloc(&dv, nout * 4));
  HIP_OK(hipMemcpy(da, a.data(), nin * 4, hipMemcpyHostToDevice)); HIP_OK(hipMemcpy(db, b.data(), nin * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemset(dm, 0xff, nout * 4)); HIP_OK(hipMemset(dv, 0xff, nout * 4));
  probe<<<256, kWave>>>(da, db, dm, dv, kCases);
  HIP_OK(hipGetLastError()); HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(om.data(), dm, nout * 4, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(ov.data(), dv, nout * 4, hipMemcpyDeviceToHost));

  // the map and the chain by a scalar triple loop on the host: quad q, row i (A's lane), column j (B's lane)
  long bad_map = 0, bad_host = 0, bad_valu = 0, transposed = 0, inexact = 0, subn = 0, total = 0;
  for (int cs = 0; cs < kCases; ++cs) {
    const float* A = &a[(size_t)cs * kTerms * kWave];
    const float* B = &b[(size_t)cs * kTerms * kWave];
    for (int q = 0; q < 16; ++q)
      for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
          float c = fmaf(A[4 * q + i], B[4 * q + j], 0.f), ct = fmaf(A[4 * q + j], B[4 * q + i], 0.f);
          bool ex = (double)A[4 * q + i] * (double)B[4 * q + j] == (double)(A[4 * q + i] * B[4 * q + j]);
          for (int t = 1; t < kTerms; ++t) {
            const float x = A[t * kWave + 4 * q + i], y = B[t * kWave + 4 * q + j];
            ex = ex && (double)x * (double)y == (double)(x * y);
            c = fmaf(x, y, c);
            ct = fmaf(A[t * kWave + 4 * q + j], B[t * kWave + 4 * q + i], ct);
          }
          const uint32_t got = bits(om[((size_t)cs * 4 + i) * kWave + 4 * q + j]), valu = bits(ov[((size_t)cs * 4 + i) * kWave + 4 * q + j]);
          const bool nan_both = std::isnan(c) && std::isnan(from_bits(got));
          ++total;
          inexact += ex ? 0 : 1;
          subn += (c != 0.f && std::fabs(c) < 1.17549435e-38f) ? 1 : 0;
          if (got != bits(c) && !nan_both) { ++bad_host; if (i != j && got == bits(ct)) ++transposed; else if (bad_map < 8) { ++bad_map; printf("case %d quad %d reg %d lane %d: mfma %08x host %08x valu %08x\n", cs, q, i, j, got, bits(c), valu); } }
          if (got != valu && !(std::isnan(from_bits(got)) && std::isnan(from_bits(valu)))) ++bad_valu;
        }
  }
  printf("mfma_gram_probe: %ld chains of %d terms (%ld with a product that needs the extra bits, %ld subnormal results)\n", total, kTerms, inexact, subn);
  printf("  mfma vs host fmaf chain: %ld differ   (of them %ld equal the TRANSPOSED element)\n", bad_host, transposed);
  printf("  mfma vs v_fma_f32 chain on the GPU: %ld differ\n", bad_valu);
  const bool ok = bad_host == 0 && bad_valu == 0;
  printf(ok ? "PASS: lane 4 q + j, register i = (A of lane 4 q + i) x (B of lane 4 q + j), one rounding per multiply-add\n" : "FAIL\n");
  return ok ? 0 : 1;
}
