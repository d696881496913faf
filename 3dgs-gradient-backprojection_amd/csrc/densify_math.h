// densify_math.h -- the arithmetic of densification (csrc/densify.hip) that is not a memory access: a step's screen-space gradient
// norm, the rule that decides what becomes of a Gaussian, and the two children of a split.
//
// All of it is float32, and the expressions below, IN THEIR WRITTEN ORDER, are the contract: nothing may be fused or
// reassociated (-ffp-contract=off), divide and sqrt are correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt), so that
// tests/densify_ref.py, the same text in numpy float32, gives the same bits.  The one exception is expf in densify_split, whose last
// bit is the library's.
//
// Plain C++: no HIP intrinsic, no header but <math.h>, so that the same text compiles for the device (csrc/densify.hip) and for the
// host (tests/densify_host.cpp).
#pragma once
#include <math.h>

#ifndef GWBP_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define GWBP_HD __host__ __device__ inline
#else
#define GWBP_HD inline
#endif
#endif

namespace gwbp {

constexpr int kDensifyPruned = 0, kDensifyKeep = 1, kDensifyClone = 2, kDensifySplit = 3; // GWBP_DENSIFY_KIND_*

// one camera's share of grad2d: the norm of the 2-D mean's gradient in units of half the image, times the number of cameras
GWBP_HD float densify_norm(float gx, float gy, float sx, float sy)
{
    const float a = gx * sx;
    const float b = gy * sy;
    return sqrtf(a * a + b * b);
}

struct DensifyThresholds { // float64 on the host, rounded to float32 once
    float t_grad;  // grow_grad2d
    float t_small; // log(grow_scale3d scene_scale)
    float t_big;   // log(prune_scale3d scene_scale)
    float t_opa;   // logit(prune_opa)
    float log16;   // log(1.6)
    int prune_big;
};

// kind of one Gaussian from its statistics and its pre-activation parameters; a comparison with a NaN is false
GWBP_HD int densify_kind(float grad2d, float count, float s0, float s1, float s2, float opacity, const DensifyThresholds &T)
{
    float m = s0;
    m = s1 > m ? s1 : m;
    m = s2 > m ? s2 : m;
    const float d = count > 1.0f ? count : 1.0f;
    const float g = grad2d / d;
    const bool low = opacity < T.t_opa;
    const bool high = g > T.t_grad;
    const bool small = m <= T.t_small;
    if (low)
        return kDensifyPruned;
    if (high && !small)
        return T.prune_big && (m - T.log16) > T.t_big ? kDensifyPruned : kDensifySplit;
    if (T.prune_big && m > T.t_big)
        return kDensifyPruned;
    return high ? kDensifyClone : kDensifyKeep;
}

GWBP_HD int densify_rows(int kind) { return kind == kDensifyPruned ? 0 : kind == kDensifyKeep ? 1 : 2; }

// child of a split: mean + R(q / |q|) (exp(scaling) * noise), q = (w, x, y, z), R as the projection builds it
GWBP_HD void densify_split(const float mean[3], const float scaling[3], const float q[4], const float noise[3], float out[3])
{
    const float n2 = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3];
    const float inv = 1.0f / sqrtf(n2);
    const float w = q[0] * inv, x = q[1] * inv, y = q[2] * inv, z = q[3] * inv;
    const float v0 = expf(scaling[0]) * noise[0];
    const float v1 = expf(scaling[1]) * noise[1];
    const float v2 = expf(scaling[2]) * noise[2];
    const float r00 = 1.0f - 2.0f * (y * y + z * z), r01 = 2.0f * (x * y - w * z), r02 = 2.0f * (x * z + w * y);
    const float r10 = 2.0f * (x * y + w * z), r11 = 1.0f - 2.0f * (x * x + z * z), r12 = 2.0f * (y * z - w * x);
    const float r20 = 2.0f * (x * z - w * y), r21 = 2.0f * (y * z + w * x), r22 = 1.0f - 2.0f * (x * x + y * y);
    out[0] = mean[0] + ((r00 * v0 + r01 * v1) + r02 * v2);
    out[1] = mean[1] + ((r10 * v0 + r11 * v1) + r12 * v2);
    out[2] = mean[2] + ((r20 * v0 + r21 * v1) + r22 * v2);
}

} // namespace gwbp
