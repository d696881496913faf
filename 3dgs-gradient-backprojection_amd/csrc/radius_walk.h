// radius_walk.h -- the ring walk that components.hip (radius components) and sample.hip (the Gaussians that weigh on a point)
// share: every point of the built grid within a radius of a query, exactly, whatever the grid.
//
// RADIUS WALK.  One lane per query.  Rings of Chebyshev radius r = 0, 1, 2, ... around the query's cell, clipped to the grid, with
// the empty-slab skip and the x-run spans of k_spatial_knn.  The lane stops after ring r when r2 < fl(LB * LB), STRICTLY, LB the
// smallest of bound_above / bound_below over the sides that still have cells, and when no side has cells left.  The argument is in
// the headers of spatial.hip (the bounds) and components.hip (the stop rule): every unvisited point has a computed d2 >= fl(LB * LB)
// > r2.  Nothing in the walk depends on which cell a point was assigned to beyond that bound, so the set of points visited with
// d2 <= r2 is the brute-force set, whatever the grid; only the ORDER of the visits depends on the grid.
#pragma once
#include "gwbp_dev.h"
#include "spatial_grid.h"

namespace gwbp {

namespace {

// The ring walk of one query: visit(d2, v, p) for every point with d2 <= r2 -- v its sorted record (x, y, z, original index), p its
// sorted position -- until it returns true ("enough") or the stop rule fires.  Returns the number of points whose distance was
// computed.
template <class Visit>
__device__ __forceinline__ int radius_walk_at(const float4 *__restrict__ S, const int32_t *__restrict__ cell_start, const SpatialGrid &G,
                                              float qx, float qy, float qz, float r2, Visit &&visit)
{
    const int nx = G.n[0], ny = G.n[1], nz = G.n[2];
    const float h = G.h;
    const int cx = cell_axis(qx, G.lo[0], h, nx), cy = cell_axis(qy, G.lo[1], h, ny), cz = cell_axis(qz, G.lo[2], h, nz);
    const float ax = qx - G.lo[0], ay = qy - G.lo[1], az = qz - G.lo[2];
    int seen = 0;
    bool enough = false;

    auto scan = [&](int b, int e) {
        for (int p = b; p < e && !enough; ++p) {
            const float4 v = S[p];
            const float dx = v.x - qx, dy = v.y - qy, dz = v.z - qz;
            const float d2 = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
            ++seen;
            if (d2 <= r2)
                enough = visit(d2, v, p);
        }
    };

    const int r_max = max(nx, max(ny, nz)); // the ring has left the grid on every side by then
    for (int r = 0; r <= r_max && !enough; ++r) {
        const int z0 = max(cz - r, 0), z1 = min(cz + r, nz - 1);
        const int y0 = max(cy - r, 0), y1 = min(cy + r, ny - 1);
        const int x0 = max(cx - r, 0), x1 = min(cx + r, nx - 1);
        for (int z = z0; z <= z1 && !enough; ++z) {
            // rows y0 .. y1 of this slab over the grid's full width hold everything the ring visits in it (k_spatial_knn's skip)
            if (cell_start[(z * ny + y0) * nx] == cell_start[(z * ny + y1) * nx + nx])
                continue;
            for (int y = y0; y <= y1 && !enough; ++y) {
                const int base = (z * ny + y) * nx;
                if (abs(z - cz) == r || abs(y - cy) == r) { // the whole run along x lies in the ring
                    scan(cell_start[base + x0], cell_start[base + x1 + 1]);
                } else { // (r > 0) only the two ends do
                    if (cx - r >= 0)
                        scan(cell_start[base + cx - r], cell_start[base + cx - r + 1]);
                    if (cx + r <= nx - 1)
                        scan(cell_start[base + cx + r], cell_start[base + cx + r + 1]);
                }
            }
        }
        // what is left lies r + 1 cells or more away along some axis: the smallest bound over the sides that still have cells
        float lb = __builtin_inff();
        bool any = false;
        if (cx + r + 1 <= nx - 1) {
            lb = fminf(lb, bound_above(ax, cx + r + 1, h));
            any = true;
        }
        if (cx - r - 1 >= 0) {
            lb = fminf(lb, bound_below(ax, cx - r, h));
            any = true;
        }
        if (cy + r + 1 <= ny - 1) {
            lb = fminf(lb, bound_above(ay, cy + r + 1, h));
            any = true;
        }
        if (cy - r - 1 >= 0) {
            lb = fminf(lb, bound_below(ay, cy - r, h));
            any = true;
        }
        if (cz + r + 1 <= nz - 1) {
            lb = fminf(lb, bound_above(az, cz + r + 1, h));
            any = true;
        }
        if (cz - r - 1 >= 0) {
            lb = fminf(lb, bound_below(az, cz - r, h));
            any = true;
        }
        if (!any || r2 < lb * lb)
            break;
    }
    return seen;
}

// the walk as the components kernels use it: visit(d2, id), id the point's original index
template <class Visit>
__device__ __forceinline__ int radius_walk(const float4 *__restrict__ S, const int32_t *__restrict__ cell_start, const SpatialGrid &G,
                                           float qx, float qy, float qz, float r2, Visit &&visit)
{
    return radius_walk_at(S, cell_start, G, qx, qy, qz, r2, [&](float d2, const float4 &v, int) { return visit(d2, __float_as_int(v.w)); });
}

} // namespace

} // namespace gwbp
