// rt_f64.h — f64 sqrt and reciprocal without the range scaling and special-case fix-up, for arguments
// known to lie well inside the exponent range (device code only).
//
// What the compiler makes of sqrt(double) and 1.0 / x on gfx950 (make asm) is a core with a shell
// around it:
//   sqrt:  x < 2^-767 ? scale x by 2^256 : by 1 (v_cmp_gt_f64, v_cndmask, v_ldexp_f64); the core below on the
//          scaled x; the result scaled by 2^-128 or 1 (v_cndmask, v_ldexp_f64); +-0 and +inf passed
//          through instead (v_cmp_class_f64, two v_cndmask).
//   1 / x: denominator and numerator scaled by v_div_scale_f64; the core below on the scaled pair, its
//          last step by v_div_fmas_f64 (an fma, times a power of two when VCC says the numerator was
//          scaled); v_div_fixup_f64 for 0, inf, nan and quotients next to the subnormal range.
// Exactness, once, for x with f64_mid(x), i.e. finite, positive, 2^-256 <= x < 2^256:
//   sqrt:  x >= 2^-767, so both scale exponents are 0 and v_ldexp_f64 by 0 returns its operand; x is
//          neither zero nor infinite, so the class select keeps the core's value.
//   1 / x: v_div_scale_f64 scales only where the denominator is subnormal, 1 / x is subnormal
//          (x > 2^1022), the exponents of numerator and denominator differ by 768 or more (x < 2^-767
//          for the numerator 1), the quotient is subnormal, or the numerator's exponent is 53 or less.
//          None holds, so both results are the operands, VCC is clear and v_div_fmas_f64 is the plain
//          fma; v_div_fixup_f64 replaces its first operand only for nan, inf, zero and out-of-range
//          cases and otherwise gives it the sign of the quotient, which is +.
// So sqrt_core / rcp_core give the bits of sqrt(x) / (1.0 / x), the IEEE results, on that window, whose
// margin to every threshold above is more than 500 binades.  sqrt_mid / rcp_mid branch to the plain forms
// for every other x (zero, subnormal, negative, huge, inf, nan) and so equal them for every input.
// sqrt maps the window into [2^-128, 2^128), again inside it: the guard of 1 / sqrt(x) follows from x's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rtamd {

// the core of sqrt(double): v_rsq_f64, then Goldschmidt's coupled step and two residual corrections
__device__ __forceinline__ double sqrt_core(const double x) {
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y, h = y * 0.5;
    const double r = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, r, g);
    h = __builtin_fma(h, r, h);
    double d = __builtin_fma(-g, g, x);
    g = __builtin_fma(d, h, g);
    d = __builtin_fma(-g, g, x);
    return __builtin_fma(d, h, g);
}
// the core of 1.0 / x: v_rcp_f64, two Newton steps, the quotient 1 * r and its residual correction
// (the product by the unscaled numerator 1.0 is exact and folds away)
__device__ __forceinline__ double rcp_core(const double x) {
    double r = __builtin_amdgcn_rcp(x);
    double e = __builtin_fma(-x, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-x, r, 1.0);
    r = __builtin_fma(r, e, r);
    const double q = 1.0 * r;
    return __builtin_fma(__builtin_fma(-x, q, 1.0), r, q);
}

// 2^-256 <= x < 2^256, finite and positive: one unsigned compare on the high word (sign 0, biased
// exponent in [1023 - 256, 1023 + 256))
constexpr uint32_t kF64MidLo = (1023u - 256u) << 20, kF64MidSpan = 512u << 20;
__device__ __forceinline__ bool f64_mid(const double x) {
    return (uint32_t)__double2hiint(x) - kF64MidLo < kF64MidSpan;
}
// sqrt(x) and 1.0 / x for every x; the core inside the window, the plain form on a rarely taken branch
__device__ __forceinline__ double sqrt_mid(const double x) {
    if (__builtin_expect(f64_mid(x), 1)) return sqrt_core(x);
    return sqrt(x);
}
__device__ __forceinline__ double rcp_mid(const double x) {
    if (__builtin_expect(f64_mid(x), 1)) return rcp_core(x);
    return 1.0 / x;
}

}  // namespace rtamd
