// nmf_exact.h — device arithmetic that the library's fast-math flags must not touch: what the sensory stages (nmf_taxis.hip,
// nmf_motion.hip) share so that kernel and numpy specification agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>

namespace nmf {

// x / y correctly rounded.  The library is compiled with -fapprox-func, under which a double division — and so __ddiv_rn, which
// the headers define as a plain one — becomes a refined reciprocal times x with neither scaling nor fix-up, a unit in the last
// place off now and then; no pragma takes that licence back on this target.  So the division is spelt out: the instruction
// sequence the compiler emits for an IEEE division (checked against it instruction by instruction).
__device__ __forceinline__ double div_rn(double x, double y) {
#pragma clang fp contract(off) reassociate(off)
  bool scaled, unused;
  const double ys = __builtin_amdgcn_div_scale(x, y, false, &unused);      // the denominator, scaled into range
  const double xs = __builtin_amdgcn_div_scale(x, y, true, &scaled);       // the numerator
  const double r0 = __builtin_amdgcn_rcp(ys);
  const double r1 = __builtin_fma(r0, __builtin_fma(-ys, r0, 1.0), r0);
  const double r2 = __builtin_fma(r1, __builtin_fma(-ys, r1, 1.0), r1);
  const double q0 = xs * r2;
  return __builtin_amdgcn_div_fixup(__builtin_amdgcn_div_fmas(__builtin_fma(-ys, q0, xs), r2, q0, scaled), y, x);
}

// v with a zero of either sign turned into +0, in integer arithmetic: the library's -fno-signed-zeros lets the compiler choose the
// sign of a floating-point zero, and no floating-point licence touches this.
__device__ __forceinline__ float plus_zero(float v) {
  const unsigned int bits = __float_as_uint(v);
  return __uint_as_float((bits << 1) == 0u ? 0u : bits);
}

}  // namespace nmf
