// spatial_grid.h -- the uniform grid that spatial.hip (k nearest neighbours), components.hip (radius components) and sample.hip
// share: the grid itself, THE cell assignment, and the lower bounds of the ring walk's stop rule.  The derivation of the bounds is in
// the header of ring_walk.h; the stop rule rests on it, and on every kernel using this one cell expression.
#pragma once
#include "gwbp_dev.h"

namespace gwbp {

namespace {

struct SpatialGrid {
    float lo[3];
    float h;
    int n[3];
};

__device__ __forceinline__ bool finite3(float x, float y, float z)
{
    return fabsf(x) < __builtin_inff() && fabsf(y) < __builtin_inff() && fabsf(z) < __builtin_inff(); // false for NaN
}

// THE cell assignment (see the header of spatial.hip for the grid): every kernel and the stop rule's derivation use this one expression.
__device__ __forceinline__ int cell_axis(float x, float lo, float h, int n)
{
    const float t = floorf((x - lo) / h);
    return (int)fminf(fmaxf(t, 0.0f), (float)(n - 1)); // (finite x: an overflowed difference is +-inf, and clamps to a border cell)
}

// lower bounds of the stop rule (header of ring_walk.h): on the distance along one axis to any point in a cell >= kf / in a cell < kf
__device__ __forceinline__ float bound_above(float A, int kf, float h)
{
    const float KH = (float)kf * h;
    const float LB = (KH - A) - (fabsf(KH) + fabsf(A)) * 0x1p-21f;
    return LB > 0.0f ? LB : 0.0f;
}
__device__ __forceinline__ float bound_below(float A, int kf, float h)
{
    const float KH = (float)kf * h;
    const float LB = (A - KH) - (fabsf(KH) + fabsf(A)) * 0x1p-21f;
    return LB > 0.0f ? LB : 0.0f;
}

[[maybe_unused]] SpatialGrid make_grid(const float *lo, float h, const int32_t *dims)
{
    SpatialGrid G;
    for (int a = 0; a < 3; ++a) {
        G.lo[a] = lo[a];
        G.n[a] = dims[a];
    }
    G.h = h;
    return G;
}

} // namespace

} // namespace gwbp
