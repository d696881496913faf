// ssim_math.h -- the arithmetic of the photometric loss (csrc/ssim.hip) that is not a memory access: the window, the chain of a
// blur, the pointwise SSIM with its three partial derivatives, and the combination that yields the gradient of a pixel.
//
// All of it is float32, and the expressions below, IN THEIR WRITTEN ORDER, are the contract: nothing may be fused or
// reassociated (-ffp-contract=off; the fused multiply-adds of a chain are written as fmaf).
//
// Plain C++: no HIP intrinsic, no header but <math.h>, so that the same text compiles for the device (csrc/ssim.hip) and for the host
// (tests/ssim_host.cpp, where it is checked against float64).
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

constexpr int kSsimWin = 11, kSsimHalo = 5;
// g[i] = exp(-(i - 5)^2 / (2 1.5^2)), i = 0 .. 10, normalised to sum 1 in float64 and rounded to float32 once
#define GWBP_SSIM_WINDOW                                                                                                             \
    {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c4p-3f, 0x1.10656p-2f,                                   \
     0x1.b43c4p-3f,   0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f}
constexpr float kSsimC1 = 0x1.a36e2ep-14f; // 0.01^2 (float64), rounded to float32
constexpr float kSsimC2 = 0x1.d7dbf4p-11f; // 0.03^2

// one step of a blur chain: acc = fmaf(g[i], v, acc), i ascending, acc starts at +0; a pixel outside the image is v = +0
GWBP_HD float ssim_chain(float g, float v, float acc) { return fmaf(g, v, acc); }

struct SsimPoint {
    float ssim; // (A B) / (Cn Dn)
    float dmu;  // d ssim / d mu1 in total, with m2 and m4 held fixed
    float d1;   // d ssim / d s1
    float d12;  // d ssim / d s12
};

// m0 .. m4: the blurs of x, y, x x, y y, x y at one window
GWBP_HD SsimPoint ssim_point(float m0, float m1, float m2, float m3, float m4)
{
    const float mu1 = m0, mu2 = m1;
    const float s1 = m2 - mu1 * mu1;
    const float s2 = m3 - mu2 * mu2;
    const float s12 = m4 - mu1 * mu2;
    const float A = (2.0f * mu1) * mu2 + kSsimC1;
    const float B = 2.0f * s12 + kSsimC2;
    const float Cn = (mu1 * mu1 + mu2 * mu2) + kSsimC1;
    const float Dn = (s1 + s2) + kSsimC2;
    const float ab = A * B;
    const float cd = Cn * Dn;
    SsimPoint P;
    P.ssim = ab / cd;
    P.d12 = (2.0f * A) / cd;
    P.d1 = -ab / (cd * Dn);
    P.dmu = (((2.0f * mu2) * B) / cd - ((2.0f * mu1) * ab) / (Cn * cd) - (2.0f * mu1) * P.d1) - mu2 * P.d12;
    return P;
}

// the gradient of one element: a, b, c are the blurs of w dmu, w d1, w d12; s_s = -lambda / (D Wv), s_1 = (1 - lambda) / (D Wa)
GWBP_HD float ssim_grad(float x, float y, float w, float a, float b, float c, float s_s, float s_1)
{
    const float e = x - y;
    const float sgn = e > 0.0f ? 1.0f : e < 0.0f ? -1.0f : 0.0f; // sign(0) = 0; a NaN difference gives 0 here and NaN below
    return s_s * ((a + (2.0f * x) * b) + y * c) + (s_1 * w) * sgn;
}

} // namespace gwbp
