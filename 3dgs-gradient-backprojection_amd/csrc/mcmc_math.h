// mcmc_math.h -- the arithmetic of the MCMC strategy (csrc/mcmc.hip; gsplat's MCMCStrategy) that is not a memory
// access: the integer sampling weight of a Gaussian, the opacity and scale of a parent that was drawn `ratio - 1` times, and the
// per-step noise on a mean.
//
// All of it is float32, and the expressions below, IN THEIR WRITTEN ORDER, are the contract: nothing may be fused or reassociated
// (-ffp-contract=off), divide and sqrt are correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt), so that tests/mcmc_ref.py,
// the same text in numpy float32, gives the same bits.  The exceptions are the library's: expf and logf of the activations and the one
// powf of mcmc_relocate, whose last bits are the library's (the restatement takes their values as arguments).
//
// Plain C++: no HIP intrinsic, no header but <math.h> and <stdint.h>, so that the same text compiles for the device (csrc/mcmc.hip) and
// for the host (tests/mcmc_host.cpp).
#pragma once
#include <math.h>
#include <stdint.h>

#include "densify_math.h" // GWBP_HD

namespace gwbp {

constexpr int kMcmcMaxRatio = 51;                 // GWBP_MCMC_MAX_RATIO: gsplat's n_max
constexpr float kMcmcWeightScale = 16777216.0f;   // 2^24: the weights are floor(sigmoid 2^24)
constexpr float kMcmcOpacityMax = 0x1.fffffcp-1f; // 1 - 2^-23 = 1 - eps(float32), the upper clamp of a relocated opacity

// binomial coefficients C(n, k), n, k < 51, each the exact integer rounded to float32 once (C(50, 25) needs 47 bits)
struct McmcBinomials {
    float c[kMcmcMaxRatio][kMcmcMaxRatio];
};

constexpr McmcBinomials mcmc_binomials()
{
    unsigned long long e[kMcmcMaxRatio][kMcmcMaxRatio] = {};
    McmcBinomials B = {};
    for (int n = 0; n < kMcmcMaxRatio; ++n)
        for (int k = 0; k <= n; ++k) {
            e[n][k] = (k == 0 || k == n) ? 1ull : e[n - 1][k - 1] + e[n - 1][k];
            B.c[n][k] = (float)e[n][k];
        }
    return B;
}

#if defined(__HIP_DEVICE_COMPILE__)
__device__ const McmcBinomials kMcmcBinomials = mcmc_binomials();
#else
static constexpr McmcBinomials kMcmcBinomials = mcmc_binomials();
#endif

GWBP_HD float mcmc_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// the integer sampling weight: 0 for a dead Gaussian (the comparison is in pre-activation space and false with a NaN), else
// floor(sigmoid(opacity) 2^24).  t_opa = -inf keeps the weight of every Gaussian but a NaN's.
GWBP_HD int64_t mcmc_weight(float opacity_logit, float t_opa)
{
    if (!(opacity_logit > t_opa))
        return 0;
    return (int64_t)floorf(mcmc_sigmoid(opacity_logit) * kMcmcWeightScale);
}

// A parent of `ratio` Gaussians (itself and ratio - 1 copies, ratio in [1, kMcmcMaxRatio]):
//   o' = 1 - (1 - o)^(1 / ratio),   s' = s (o / D),   D = sum_{i = 1..ratio} sum_{k = 0..i-1} C(i-1, k) (-1)^k o'^(k+1) / sqrt(k + 1)
// D takes the unclamped o'; what is returned is clamped to [min_opacity, 1 - eps] and in pre-activation form (logit, log).
GWBP_HD void mcmc_relocate(float opacity_logit, const float scaling[3], int ratio, float min_opacity, float *out_opacity, float out_scaling[3])
{
    const float o = mcmc_sigmoid(opacity_logit);
    const float inv_ratio = 1.0f / (float)ratio;
    const float on = 1.0f - powf(1.0f - o, inv_ratio);
    float denom = 0.0f;
    for (int i = 1; i <= ratio; ++i) {
        float p = on, sign = 1.0f;
        for (int k = 0; k < i; ++k) {
            const float inv_sqrt = 1.0f / sqrtf((float)(k + 1));
            denom = denom + ((kMcmcBinomials.c[i - 1][k] * sign) * p) * inv_sqrt;
            p = p * on;
            sign = -sign;
        }
    }
    const float coeff = o / denom;
    float oc = on;
    oc = oc < min_opacity ? min_opacity : oc;
    oc = oc > kMcmcOpacityMax ? kMcmcOpacityMax : oc;
    *out_opacity = logf(oc / (1.0f - oc));
    out_scaling[0] = logf(expf(scaling[0]) * coeff);
    out_scaling[1] = logf(expf(scaling[1]) * coeff);
    out_scaling[2] = logf(expf(scaling[2]) * coeff);
}

// how much of the noise a Gaussian of this opacity takes: g(1 - o), g(x) = 1 / (1 + exp(-100 (x - 0.995)))
GWBP_HD float mcmc_gate(float opacity_logit)
{
    const float o = mcmc_sigmoid(opacity_logit);
    const float x = 1.0f - o;
    return 1.0f / (1.0f + expf(-100.0f * (x - 0.995f)));
}

// mean + Sigma v,  Sigma = R diag(exp(2 s)) R^T,  v = z g scaler;  R of q / |q|, q = (w, x, y, z), as densify_split builds it
GWBP_HD void mcmc_noise(const float mean[3], const float scaling[3], const float q[4], float opacity_logit, const float z3[3], float scaler,
                        float out[3])
{
    const float n2 = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3];
    const float inv = 1.0f / sqrtf(n2);
    const float w = q[0] * inv, x = q[1] * inv, y = q[2] * inv, z = q[3] * inv;
    const float r00 = 1.0f - 2.0f * (y * y + z * z), r01 = 2.0f * (x * y - w * z), r02 = 2.0f * (x * z + w * y);
    const float r10 = 2.0f * (x * y + w * z), r11 = 1.0f - 2.0f * (x * x + z * z), r12 = 2.0f * (y * z - w * x);
    const float r20 = 2.0f * (x * z - w * y), r21 = 2.0f * (y * z + w * x), r22 = 1.0f - 2.0f * (x * x + y * y);
    const float g = mcmc_gate(opacity_logit);
    const float v0 = (z3[0] * g) * scaler, v1 = (z3[1] * g) * scaler, v2 = (z3[2] * g) * scaler;
    const float t0 = expf(2.0f * scaling[0]) * ((r00 * v0 + r10 * v1) + r20 * v2);
    const float t1 = expf(2.0f * scaling[1]) * ((r01 * v0 + r11 * v1) + r21 * v2);
    const float t2 = expf(2.0f * scaling[2]) * ((r02 * v0 + r12 * v1) + r22 * v2);
    out[0] = mean[0] + ((r00 * t0 + r01 * t1) + r02 * t2);
    out[1] = mean[1] + ((r10 * t0 + r11 * t1) + r12 * t2);
    out[2] = mean[2] + ((r20 * t0 + r21 * t1) + r22 * t2);
}

} // namespace gwbp
