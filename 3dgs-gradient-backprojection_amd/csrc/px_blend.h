// px_blend.h -- one Gaussian record at one pixel, as the pixel-parallel tile rasterisers blend it (k_render_px in render.hip,
// k_render_labels in label_render.hip): workgroup = 16x16 tile, thread = pixel, records staged in LDS per batch of 256.  The
// expressions are k_blend's, so alpha / T / early termination are bit-identical in every kernel that includes this header; they
// are written ONCE here so that no kernel can drift from the others.
#pragma once
#include "gwbp_dev.h"

namespace gwbp {
#ifdef __HIPCC__

// The first 16 B of a projected record {mx, my, opac, depth} as the loop reads them: {mx, my, opac, ln(255 opac) + margin}.
// alpha = o exp(-sigma) >= 1/255  <=>  sigma <= ln(255 o); 1e-3 absorbs the error of __logf and exp_neg (k_blend's s_thr);
// o <= 1/255 gives a negative bound that no sigma >= 0 meets.
__device__ __forceinline__ float4 px_stage(float4 a)
{
    a.w = __logf(255.0f * a.z) + 1e-3f;
    return a;
}

// a = {mx, my, opac, bound}, b = {ca, cb, cc, -}
__device__ __forceinline__ float px_sigma(const float4 &a, const float4 &b, float px, float py)
{
    const float dx = a.x - px, dy = a.y - py;
    return __builtin_fmaf(b.y * dx, dy, 0.5f * __builtin_fmaf(b.x * dx, dx, (b.z * dy) * dy));
}

// Wave-uniform: no live pixel of this wave's 4 x 16 quarter lies inside the record's alpha >= 1/255 ellipse (skips exp and T;
// changes no bit: sigma above ln(255 o) + margin cannot reach 1/255).
__device__ __forceinline__ bool px_quarter_outside(bool done, float sigma, float bound)
{
    return __ballot(!done && sigma <= bound) == 0ull;
}

// Advances the pixel's T / done by the record and returns whether the record contributes; w = alpha * T of a contributing
// record, 0 otherwise.  An accumulator takes the record under `valid ? ... : ...`, never as a w = 0 product (a non-finite
// payload must reach only the pixels the record has a weight at).
__device__ __forceinline__ bool px_step(float sigma, float opac, float &T, bool &done, float &w)
{
    const float alpha = __builtin_fminf(kAlphaMax, opac * exp_neg(-__builtin_fmaxf(sigma, 0.f)));
    const bool ok = !done && (sigma >= 0.f) && (alpha >= kAlphaMin);
    const float next_T = T * (1.0f - alpha);
    const bool term = ok && (next_T <= kTMin);
    const bool valid = ok && !term;
    w = valid ? alpha * T : 0.f;
    T = valid ? next_T : T;
    done = done || term;
    return valid;
}

// The record's alpha at a pixel as px_step computes it (the same expression: the same bits), with its two factors: vis = exp(-sigma)
// and raw = opac * vis, the value before the clamp at kAlphaMax.  For the walk back over a pixel's list (k_render_px_bwd), which
// needs d(alpha) / d(sigma, opac) and has no T / done to advance.
__device__ __forceinline__ float px_alpha(float sigma, float opac, float &vis, float &raw)
{
    vis = exp_neg(-__builtin_fmaxf(sigma, 0.f));
    raw = opac * vis;
    return __builtin_fminf(kAlphaMax, raw);
}

// Wave-uniform: nobody in the wave takes anything from this record (skips the payload's reads and adds).
__device__ __forceinline__ bool px_nobody(bool valid) { return __ballot(valid) == 0ull; }

#endif
} // namespace gwbp
