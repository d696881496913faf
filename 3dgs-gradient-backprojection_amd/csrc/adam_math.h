// adam_math.h -- the update of ONE element under Adam (csrc/adam.hip; torch.optim.Adam with weight_decay = 0, amsgrad = False,
// maximize = False).
//
// All of it is float32, and the expressions below, IN THEIR WRITTEN ORDER, are the contract: nothing is fused or reassociated
// (-ffp-contract=off; there is no fmaf in this file), divide and sqrtf are correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt),
// so that tests/adam_ref.py, the same text in numpy float32, gives the same bits:
//
//     d     = g - m
//     m'    = m + one_minus_b1 * d                    (torch: exp_avg.lerp_(grad, 1 - beta1), a weight below 0.5)
//     v'    = b2 * v + (one_minus_b2 * g) * g         (torch: exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2))
//     denom = sqrtf(v') / sqrt_bc2 + eps
//     p'    = p - step_size * (m' / denom)            (torch: param.addcdiv_(exp_avg, denom, value = -step_size))
//
// The five scalars are the HOST's: each is computed in float64 and rounded to float32 ONCE (AdamScalars::make below) --
// one_minus_b1 = 1 - b1 and one_minus_b2 = 1 - b2 from the float64 betas (1 - 0.999 formed from a float32 0.999 would be off by 5e-5 of
// itself), step_size = lr / (1 - b1^t) and sqrt_bc2 = sqrt(1 - b2^t) as the caller hands them in.  Nothing is read back from the device.
//
// g == 0 with m == v == 0 leaves the bits of p, m and v: d = +-0, m' = +0 + (+-0) = +0, v' = +0 + (+-0)(+-0) = +0, denom = eps,
// m' / denom = +0 and p - step_size (+0) = p - (+-0) = p, also for p = -0 (what DESIGN.md 4.0k relies on for the SH rows above a step's
// degree).  eps > 0 is the caller's to keep: with eps = 0 that quotient is 0 / 0.  Denormal operands and results follow the target's
// float32 denormal mode and are not part of the contract.
//
// Plain C++: no HIP intrinsic, no header but <math.h>, so that the same text compiles for the device (csrc/adam.hip) and for the host
// (tests/adam_host.cpp).
#pragma once
#include <math.h>

#include "densify_math.h" // GWBP_HD

namespace gwbp {

struct AdamScalars {
    float step_size, sqrt_bc2, one_minus_b1, b2, one_minus_b2, eps;

    // the float64 -> float32 roundings, once each, in one place
    static inline AdamScalars make(float lr_over_bc1, float sqrt_bc2, double b1, double b2, float eps)
    {
        return AdamScalars{lr_over_bc1, sqrt_bc2, (float)(1.0 - b1), (float)b2, (float)(1.0 - b2), eps};
    }
};

GWBP_HD void adam_element(float &p, float g, float &m, float &v, const AdamScalars &S)
{
    const float d = g - m;
    const float m1 = m + S.one_minus_b1 * d;
    const float v1 = S.b2 * v + (S.one_minus_b2 * g) * g;
    const float denom = sqrtf(v1) / S.sqrt_bc2 + S.eps;
    p = p - S.step_size * (m1 / denom);
    m = m1;
    v = v1;
}

} // namespace gwbp
