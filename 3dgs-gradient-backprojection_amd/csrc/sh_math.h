// sh_math.h -- the arithmetic of the SH colours and of their backward (csrc/sh.hip) that is not a memory access: the
// view direction of a Gaussian, the real SH basis up to degree 3 and its derivatives, the colour chain of k_sh_colors (csrc/render.hip)
// and the gradients w.r.t. the coefficients and the mean.
//
// All of it is float32, and the expressions below, IN THEIR WRITTEN ORDER, are the contract: nothing may be fused or reassociated
// (-ffp-contract=off), the FMAs are the written fmaf calls, divide and sqrt are correctly rounded
// (-fhip-fp32-correctly-rounded-divide-sqrt).  The forward is k_sh_colors' chain and gives its bits.  The backward differentiates
// projection.sh_colors_torch, its two kinks included: a channel passes its gradient where the forward's own pre-clamp value r
// satisfies r + 0.5f >= 0 (torch's clamp_min rule; a NaN passes nothing), and a Gaussian closer than 1e-12 to the camera centre takes
// the clamp's branch of the normalisation (dir = d 1e12, no projection term).
//
// Plain C++: no HIP intrinsic, no header but <math.h>, so that the same text compiles for the device (csrc/sh.hip) and for the host
// (tests/sh_host.cpp).
#pragma once
#include <math.h>

#include "densify_math.h" // GWBP_HD

#if defined(__clang__)
#define GWBP_SH_UNROLL _Pragma("unroll")
#elif defined(__GNUC__)
#define GWBP_SH_UNROLL _Pragma("GCC unroll 16")
#else
#define GWBP_SH_UNROLL
#endif

namespace gwbp {

constexpr int kShMaxDegree = 3;
constexpr int kShMaxBasis = 16; // GWBP_SH_MAX_K: (kShMaxDegree + 1)^2, the widest coefficient row
constexpr float kShC0 = 0.28209479177387814f;
constexpr float kShC1 = 0.4886025119029199f;
constexpr float kShC20 = 1.0925484305920792f, kShC21 = 0.31539156525252005f, kShC22 = 0.5462742152960396f;
constexpr float kShC30 = 0.5900435899266435f, kShC31 = 2.890611442640554f, kShC32 = 0.4570457994644658f, kShC33 = 0.3731763325901154f,
                kShC34 = 1.445305721320277f;
constexpr float kShMinNorm = 1e-12f;

struct ShDir {
    float x, y, z; // d / max(|d|, 1e-12)
    float inv;     // 1 / max(|d|, 1e-12)
    bool clamped;  // |d| <= 1e-12: the direction is d 1e12 and its norm does not depend on d
};

GWBP_HD ShDir sh_direction(const float mean[3], float cx, float cy, float cz)
{
    float x = mean[0] - cx, y = mean[1] - cy, z = mean[2] - cz;
    const float n = sqrtf(x * x + y * y + z * z);
    const float inv = 1.0f / fmaxf(n, kShMinNorm);
    x *= inv, y *= inv, z *= inv;
    return ShDir{x, y, z, inv, !(n > kShMinNorm)};
}

// b[0 .. (DEG + 1)^2): the basis expressions of k_sh_colors, unchanged
template <int DEG> GWBP_HD void sh_basis(float x, float y, float z, float b[kShMaxBasis])
{
    b[0] = kShC0;
    if (DEG >= 1) {
        b[1] = -kShC1 * y, b[2] = kShC1 * z, b[3] = -kShC1 * x;
    }
    if (DEG >= 2) {
        const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
        b[4] = kShC20 * xy, b[5] = -kShC20 * yz;
        b[6] = kShC21 * (2.f * zz - xx - yy), b[7] = -kShC20 * xz;
        b[8] = kShC22 * (xx - yy);
        if (DEG >= 3) {
            b[9] = -kShC30 * y * (3.f * xx - yy), b[10] = kShC31 * xy * z;
            b[11] = -kShC32 * y * (4.f * zz - xx - yy);
            b[12] = kShC33 * z * (2.f * zz - 3.f * xx - 3.f * yy);
            b[13] = -kShC32 * x * (4.f * zz - xx - yy), b[14] = kShC34 * z * (xx - yy);
            b[15] = -kShC30 * x * (xx - 3.f * yy);
        }
    }
}

// the three pre-clamp sums: one fmaf chain per channel in ascending k over a row coef[k][c] of unit stride
template <int DEG> GWBP_HD void sh_preclamp(const float b[kShMaxBasis], const float *coef, float rgb[3])
{
    constexpr int NB = (DEG + 1) * (DEG + 1);
    float r = 0.f, g = 0.f, bl = 0.f;
    GWBP_SH_UNROLL
    for (int k = 0; k < NB; ++k) {
        r = fmaf(b[k], coef[3 * k], r);
        g = fmaf(b[k], coef[3 * k + 1], g);
        bl = fmaf(b[k], coef[3 * k + 2], bl);
    }
    rgb[0] = r, rgb[1] = g, rgb[2] = bl;
}

GWBP_HD float sh_clamp(float r) { return fmaxf(r + 0.5f, 0.f); }

template <int DEG> GWBP_HD void sh_forward_row(const float mean[3], float cx, float cy, float cz, const float *coef, float out[3])
{
    const ShDir d = sh_direction(mean, cx, cy, cz);
    float b[kShMaxBasis], rgb[3];
    sh_basis<DEG>(d.x, d.y, d.z, b);
    sh_preclamp<DEG>(b, coef, rgb);
    out[0] = sh_clamp(rgb[0]), out[1] = sh_clamp(rgb[1]), out[2] = sh_clamp(rgb[2]);
}

// v_dir = sum_k t[k] d b_k / d (x, y, z), the three components of the direction taken as independent variables
template <int DEG> GWBP_HD void sh_basis_backward(float x, float y, float z, const float t[kShMaxBasis], float v[3])
{
    float vx = 0.f, vy = 0.f, vz = 0.f;
    if (DEG >= 1) {
        vy = fmaf(t[1], -kShC1, vy);
        vz = fmaf(t[2], kShC1, vz);
        vx = fmaf(t[3], -kShC1, vx);
    }
    if (DEG >= 2) {
        vx = fmaf(t[4], kShC20 * y, vx), vy = fmaf(t[4], kShC20 * x, vy);
        vy = fmaf(t[5], -kShC20 * z, vy), vz = fmaf(t[5], -kShC20 * y, vz);
        vx = fmaf(t[6], -2.f * kShC21 * x, vx), vy = fmaf(t[6], -2.f * kShC21 * y, vy), vz = fmaf(t[6], 4.f * kShC21 * z, vz);
        vx = fmaf(t[7], -kShC20 * z, vx), vz = fmaf(t[7], -kShC20 * x, vz);
        vx = fmaf(t[8], 2.f * kShC22 * x, vx), vy = fmaf(t[8], -2.f * kShC22 * y, vy);
    }
    if (DEG >= 3) {
        const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
        vx = fmaf(t[9], -6.f * kShC30 * xy, vx), vy = fmaf(t[9], -3.f * kShC30 * (xx - yy), vy);
        vx = fmaf(t[10], kShC31 * yz, vx), vy = fmaf(t[10], kShC31 * xz, vy), vz = fmaf(t[10], kShC31 * xy, vz);
        vx = fmaf(t[11], 2.f * kShC32 * xy, vx), vy = fmaf(t[11], -kShC32 * (4.f * zz - xx - 3.f * yy), vy);
        vz = fmaf(t[11], -8.f * kShC32 * yz, vz);
        vx = fmaf(t[12], -6.f * kShC33 * xz, vx), vy = fmaf(t[12], -6.f * kShC33 * yz, vy);
        vz = fmaf(t[12], 3.f * kShC33 * (2.f * zz - xx - yy), vz);
        vx = fmaf(t[13], -kShC32 * (4.f * zz - 3.f * xx - yy), vx), vy = fmaf(t[13], 2.f * kShC32 * xy, vy);
        vz = fmaf(t[13], -8.f * kShC32 * xz, vz);
        vx = fmaf(t[14], 2.f * kShC34 * xz, vx), vy = fmaf(t[14], -2.f * kShC34 * yz, vy), vz = fmaf(t[14], kShC34 * (xx - yy), vz);
        vx = fmaf(t[15], -3.f * kShC30 * (xx - yy), vx), vy = fmaf(t[15], 6.f * kShC30 * xy, vy);
    }
    v[0] = vx, v[1] = vy, v[2] = vz;
}

// One Gaussian's backward.  coef: its row [K][3] of unit stride, K >= (DEG + 1)^2; v_color: d loss / d (its colour).
// v_coef (nullptr, or a row [K][3] that may be coef itself: entry k is written after it was read): b[k] v_c for k < (DEG + 1)^2 and
// +0 behind.  v_mean (nullptr, or [3]): the gradient through the direction, zeros at degree 0.
template <int DEG>
GWBP_HD void sh_backward_row(const float mean[3], float cx, float cy, float cz, const float *coef, int K, const float v_color[3],
                             float *v_coef, float *v_mean)
{
    constexpr int NB = (DEG + 1) * (DEG + 1);
    const ShDir d = sh_direction(mean, cx, cy, cz);
    float b[kShMaxBasis], rgb[3], t[kShMaxBasis];
    sh_basis<DEG>(d.x, d.y, d.z, b);
    sh_preclamp<DEG>(b, coef, rgb);
    const float v0 = rgb[0] + 0.5f >= 0.f ? v_color[0] : 0.f;
    const float v1 = rgb[1] + 0.5f >= 0.f ? v_color[1] : 0.f;
    const float v2 = rgb[2] + 0.5f >= 0.f ? v_color[2] : 0.f;
    GWBP_SH_UNROLL
    for (int k = 0; k < NB; ++k) {
        t[k] = (coef[3 * k] * v0 + coef[3 * k + 1] * v1) + coef[3 * k + 2] * v2;
        if (v_coef) {
            v_coef[3 * k] = b[k] * v0, v_coef[3 * k + 1] = b[k] * v1, v_coef[3 * k + 2] = b[k] * v2;
        }
    }
    if (v_coef)
        for (int j = 3 * NB; j < 3 * K; ++j)
            v_coef[j] = 0.f;
    if (!v_mean)
        return;
    if (DEG == 0) {
        v_mean[0] = 0.f, v_mean[1] = 0.f, v_mean[2] = 0.f;
        return;
    }
    float v[3];
    sh_basis_backward<DEG>(d.x, d.y, d.z, t, v);
    if (d.clamped) {
        v_mean[0] = v[0] * d.inv, v_mean[1] = v[1] * d.inv, v_mean[2] = v[2] * d.inv;
    } else {
        const float dot = (d.x * v[0] + d.y * v[1]) + d.z * v[2];
        v_mean[0] = (v[0] - d.x * dot) * d.inv;
        v_mean[1] = (v[1] - d.y * dot) * d.inv;
        v_mean[2] = (v[2] - d.z * dot) * d.inv;
    }
}

} // namespace gwbp
