// depth_math.h -- the arithmetic of the depth losses of training (csrc/depth_loss.hip) that is not a memory access.
//
// All of it is float32, and the expressions below, IN THEIR WRITTEN ORDER, are the contract: nothing is fused or reassociated
// (-ffp-contract=off; there is no fmaf in this file), divides are correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt), so that
// tests/depth_loss_ref.py, the same text in numpy float32, gives the same bits.  torch's grid_sample rounds differently (it normalises
// the coordinates to [-1, 1] and un-normalises them again); this chain, not that one, is what the kernels promise.
//
// A[r, c] is the accumulated depth of a render in an accumulated-depth mode, a[r, c] its alpha map.
//
//     am      = a < 1e-10f ? 1e-10f : a     (torch's clamp_min: a NaN stays one)
//     e       = A / am                      inside the image, +0 outside (grid_sample's zero padding)
//
// The point term.  (x, y) in the reference's coordinates: x is a COLUMN INDEX (column j is sampled at x = j; align_corners=True over
// x / (W - 1) * 2 - 1), half a pixel off the rasteriser's pixel centres, as the reference has it.
//
//     x0 = floorf(x), fx = x - x0, gx = 1 - fx        (y0, fy, gy likewise); the corners are (y0, x0), (y0, x0 + 1), (y0 + 1, x0), ...
//     top = gx * e00 + fx * e01
//     bot = gx * e10 + fx * e11
//     d   = gy * top + fy * bot
//     q   = d > 0 ? 1 / d : 0
//     r   = q - 1 / g
//     t   = |r|                                        loss = scale (sum t) / M, summed in float64 in a fixed order
//
// and back, with c = upstream * (float)(scale / M) (the quotient formed in float64 and rounded once):
//
//     v_d   = d > 0 ? -(sgn(r) * ((q * q) * c)) : 0    sgn(0) = 0
//     v_eij = w_ij * v_d,  w00 = gy * gx, w01 = gy * fx, w10 = fy * gx, w11 = fy * fx
//     v_A   = v_e / am
//     v_a   = a >= 1e-10f ? -((v_e * A) / (a * a)) : 0      (torch's clamp_min rule: the gradient passes where a >= the bound)
//
// Two departures from the torch expression: a sample with d <= 0 adds 1 / g to the loss and EXACT ZEROS to the gradient (torch: the
// 0 * inf of where(d > 0, 1 / d, 0) is NaN); M = 0 gives loss 0 and zero gradients (torch: NaN).  Non-finite inputs and g <= 0 are not
// masked: they propagate.
//
// The map term, per pixel, against a depth map g with an optional weight w >= 0; the pixel is valid when g > 0 (and w > 0):
//
//     disparity:  r = (e > 0 ? 1 / e : 0) - 1 / g        depth:  r = e - g
//     t   = |r|                                        loss = scale (sum w t) / (sum w) over the valid pixels, 0 without any
//     v_e = e > 0 ? -(sgn(r) * ((q * q) * (w * c))) : 0  (disparity),   e > 0 ? sgn(r) * (w * c) : 0  (depth)
//
// with c = (float)(upstream * scale / sum w) formed in float64, and v_A, v_a as above.
//
// Plain C++: no HIP intrinsic, no header but <math.h>, so that the same text compiles for the device (csrc/depth_loss.hip) and for the
// host (tests/depth_host.cpp).
#pragma once
#include <math.h>

#include "densify_math.h" // GWBP_HD

namespace gwbp {

constexpr float kDepthAlphaMin = 1e-10f;
constexpr int kDepthDisparity = 0, kDepthDepth = 1; // GWBP_DEPTH_KIND_*

GWBP_HD float depth_alpha_floor(float a) { return a < kDepthAlphaMin ? kDepthAlphaMin : a; }

// the expected depth of one pixel inside the image
GWBP_HD float depth_expected(float A, float a) { return A / depth_alpha_floor(a); }

GWBP_HD float depth_sgn(float r) { return r > 0.0f ? 1.0f : r < 0.0f ? -1.0f : 0.0f; }

// d(e) / d(A) and d(e) / d(a) applied to the gradient v_e that reaches the pixel's expected depth
GWBP_HD void depth_expected_grad(float A, float a, float v_e, float &v_A, float &v_a)
{
    v_A = v_e / depth_alpha_floor(a);
    v_a = a >= kDepthAlphaMin ? -((v_e * A) / (a * a)) : 0.0f;
}

struct DepthSample {
    float fx, fy, gx, gy; // the weights of the upper (f) and lower (g = 1 - f) corner along x and y
    float d;              // the sampled depth
    float q, r, t;        // disparity, q - 1 / g, |r|
};

// x0 = floorf(x) and y0 = floorf(y) are the caller's (they index memory); e00 .. e11 the expected depths of the four corners, +0
// for a corner outside the image
GWBP_HD DepthSample depth_sample(float x, float y, float x0, float y0, float e00, float e01, float e10, float e11, float g)
{
    DepthSample S;
    S.fx = x - x0;
    S.fy = y - y0;
    S.gx = 1.0f - S.fx;
    S.gy = 1.0f - S.fy;
    const float top = S.gx * e00 + S.fx * e01;
    const float bot = S.gx * e10 + S.fx * e11;
    S.d = S.gy * top + S.fy * bot;
    S.q = S.d > 0.0f ? 1.0f / S.d : 0.0f;
    S.r = S.q - 1.0f / g;
    S.t = fabsf(S.r);
    return S;
}

// d(loss) / d(d) of one point; c = upstream * (float)(scale / M)
GWBP_HD float depth_sample_grad(const DepthSample &S, float c) { return S.d > 0.0f ? -(depth_sgn(S.r) * ((S.q * S.q) * c)) : 0.0f; }

// the four corners' shares of v_d, in the order 00, 01, 10, 11
GWBP_HD void depth_corner_shares(const DepthSample &S, float v_d, float v_e[4])
{
    v_e[0] = (S.gy * S.gx) * v_d;
    v_e[1] = (S.gy * S.fx) * v_d;
    v_e[2] = (S.fy * S.gx) * v_d;
    v_e[3] = (S.fy * S.fx) * v_d;
}

// the map term of one valid pixel: r of the pixel's expected depth e against the map's g
GWBP_HD float depth_map_residual(int kind, float e, float g)
{
    if (kind == kDepthDepth)
        return e - g;
    const float q = e > 0.0f ? 1.0f / e : 0.0f;
    return q - 1.0f / g;
}

// d(loss) / d(e) of one valid pixel; wc = w * c with c = (float)(upstream * scale / sum w)
GWBP_HD float depth_map_grad(int kind, float e, float g, float wc)
{
    if (!(e > 0.0f))
        return 0.0f;
    const float r = depth_map_residual(kind, e, g);
    if (kind == kDepthDepth)
        return depth_sgn(r) * wc;
    const float q = 1.0f / e;
    return -(depth_sgn(r) * ((q * q) * wc));
}

} // namespace gwbp
