// The library's fp64 sigmoid without libm (K30's logistic gradient, K38's skip-gram coefficients): every step is a stated
// fp64 operation, so a numpy restatement gives the same bits.  Sources that include this are built with -ffp-contract=off.
#pragma once
#include "common.h"

namespace gae {
namespace sigma64 {

// exp(-a) for 0 <= a <= 40, the stated sequence: k = rint(-a / ln 2), r = (-a - k ln2_hi) - k ln2_lo (|r| <= 0.3466), the
// degree-13 Taylor polynomial of exp in Horner form, times 2^k built from its bits (exact)
constexpr double kInvLn2 = 1.44269504088896338700e+00, kLn2Hi = 6.93147180369123816490e-01,
                 kLn2Lo = 1.90821492927058770002e-10, kClamp = 40.0;

__device__ __forceinline__ double exp_neg(double a)
{
    const double t = -a;
    const double k = rint(t * kInvLn2);
    const double r = (t - k * kLn2Hi) - k * kLn2Lo;
    double p = 1.0 / 6227020800.0;
    p = p * r + 1.0 / 479001600.0;
    p = p * r + 1.0 / 39916800.0;
    p = p * r + 1.0 / 3628800.0;
    p = p * r + 1.0 / 362880.0;
    p = p * r + 1.0 / 40320.0;
    p = p * r + 1.0 / 5040.0;
    p = p * r + 1.0 / 720.0;
    p = p * r + 1.0 / 120.0;
    p = p * r + 1.0 / 24.0;
    p = p * r + 1.0 / 6.0;
    p = p * r + 0.5;
    p = p * r + 1.0;
    p = p * r + 1.0;
    return p * __longlong_as_double(((long long)1023 + (long long)k) << 52);
}

__device__ __forceinline__ double clamp_abs(double F)
{
    const double a = fabs(F);
    return a < kClamp ? a : kClamp;        // (a NaN takes the clamp)
}

// sigma(F) from e = exp(-min(|F|, 40)): q = e / (1 + e) is sigma(-|F|), the other side is 1 - q
__device__ __forceinline__ double sigma_of(double F, double e)
{
    const double q = e / (1.0 + e);
    return F >= 0.0 ? 1.0 - q : q;
}

__device__ __forceinline__ double sigma(double F) { return sigma_of(F, exp_neg(clamp_abs(F))); }

} // namespace sigma64
} // namespace gae
