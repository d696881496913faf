// ring_walk.h -- THE walk over the built grid of spatial_grid.h: one query's points ring by ring, nearest cells first, until a
// squared cut-off proves that nothing nearer is left.  spatial.hip (k nearest neighbours: the cut is the lane's k-th d2 so far),
// components.hip (radius components) and sample.hip (the Gaussians that weigh on a point) -- both with a fixed cut r2 -- share it.
//
//   d2(p, q) = fmaf(dz, dz, fmaf(dy, dy, dx * dx)),  dx = p.x - q.x (fp32)
//
// THE WALK.  One lane per query.  Rings of Chebyshev radius r = 0, 1, 2, ... around the query's cell, clipped to the grid; within a
// ring every run of cells along x is one contiguous span of the sorted points (inside the ring's box only the two end cells of a
// run belong to the ring).  Rows y0 .. y1 of a slab over the grid's full width hold everything the ring visits in that slab:
// nothing there, nothing to visit (a floater in a border cell crosses the empty part of the grid in O(r) steps per ring, not
// O(r^2)).  No lane waits for another lane or workgroup.  The trip count is at most max(nx, ny, nz) + 1.
//
// STOP RULE, and why it is exact although points are assigned to cells by a ROUNDED expression.  After ring r every unvisited
// point p sits in a cell that differs from the query's by at least r + 1 along some axis, say cell(p) >= kf = cq + r + 1 (the
// other side is symmetric).  Clamping only lowers a cell index from above, so the unclamped t(p) >= kf as well, i.e. the rounded
// quotient u = fl(fl(p.x - lo) / h) >= kf.  A subtraction and a correctly rounded division are each within a factor
// (1 +- 2^-24) of the exact result, so in exact arithmetic
//       p.x - lo  >=  kf * h / (1 + 2^-24)^2  >=  kf * h * (1 - 2^-22).
// This bounds the point's position relative to lo by the FACE's position, whatever the magnitude of p.x: the error of the
// assignment is an ulp of |x - lo| scaled to cell units, not an ulp of the bound.  The exact distance along that axis is then
//       (p.x - lo) - (q.x - lo)  >=  kf * h * (1 - 2^-22) - a,        a = q.x - lo.
// In fp32: A = fl(q.x - lo) (|A - a| <= 2^-24 |a|), KH = fl(kf * h) (kf <= 1024 is exact, |KH - kf h| <= 2^-24 kf h),
// B = fl(KH - A) (|B - (KH - A)| <= 2^-24 (KH + |A|)).  Together the exact bound is at least
//       B - [ KH (2^-22 + 2^-23) + |A| 2^-23 ] (1 + small)   >   B - (KH + |A|) * 0.75 * 2^-21,
// and LB = fl(B - fl((KH + |A|) * 2^-21)) keeps the remaining quarter for its own two roundings (bound_above / bound_below of
// spatial_grid.h).  A non-positive or NaN LB becomes 0 ("no bound").  The margin errs towards one more ring, never towards stopping.
// From an exact |p.x - q.x| >= LB with LB a float, rounding being monotone gives |dx| = |fl(p.x - q.x)| >= LB, then
// fl(dx * dx) >= fl(LB * LB), and each fmaf adds a non-negative term before a monotone rounding: the COMPUTED d2(p, q) >= fl(LB *
// LB), whichever axis carried the bound.  The lane stops after ring r when cut() is STRICTLY below fl(LB * LB), LB the smallest
// bound over the (up to six) directions that still have cells: every unvisited point then has a computed d2 > cut().  (Strictly:
// the callers count a point at exactly the cut.)  A direction whose next ring has left the grid has no points (its bound is
// infinite); when all six have, everything has been visited.  Nothing in the walk depends on which cell a point was assigned to
// beyond that bound, so the set of points visited with d2 <= the final cut is the brute-force set, whatever the grid; only the
// ORDER of the visits depends on the grid.
#pragma once
#include <type_traits>

#include "gwbp_dev.h"
#include "spatial_grid.h"

namespace gwbp {

namespace {

// The walk of one query.  visit(d2, v, p) for every scanned point -- v its sorted record (x, y, z, original index), p its sorted
// position; cut() is the squared cut-off, read after each ring.  A visitor that returns bool ends the walk by returning true
// ("enough"); one that returns void compiles to loops without that test.  Returns the number of points scanned.
template <class Cut, class Visit>
__device__ __forceinline__ int ring_walk(const float4 *__restrict__ S, const int32_t *__restrict__ cell_start, const SpatialGrid &G,
                                         float qx, float qy, float qz, Cut cut, Visit visit)
{
    constexpr bool kExit = !std::is_void_v<decltype(visit(0.0f, S[0], 0))>;
    const int nx = G.n[0], ny = G.n[1], nz = G.n[2];
    const float h = G.h;
    const int cx = cell_axis(qx, G.lo[0], h, nx), cy = cell_axis(qy, G.lo[1], h, ny), cz = cell_axis(qz, G.lo[2], h, nz);
    const float ax = qx - G.lo[0], ay = qy - G.lo[1], az = qz - G.lo[2];
    int seen = 0;
    [[maybe_unused]] bool enough = false;
    auto go_on = [&] { // part of every loop's condition: the exit test, only where the visitor can ask for one
        if constexpr (kExit)
            return !enough;
        else
            return true;
    };

    auto scan = [&](int b, int e) {
        for (int p = b; p < e && go_on(); ++p) {
            const float4 v = S[p];
            const float dx = v.x - qx, dy = v.y - qy, dz = v.z - qz;
            const float d2 = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
            ++seen;
            if constexpr (kExit)
                enough = visit(d2, v, p);
            else
                visit(d2, v, p);
        }
    };

    // the ring has left the grid on every side by then.  uniform(): the bound is the same in every lane, and saying so keeps it and
    // the ring loop's own exit test in scalar registers (without it the compiler folds that test into the lanes' stop condition)
    const int r_max = (int)uniform((u32)max(nx, max(ny, nz)));
    for (int r = 0; r <= r_max && go_on(); ++r) {
        const int z0 = max(cz - r, 0), z1 = min(cz + r, nz - 1);
        const int y0 = max(cy - r, 0), y1 = min(cy + r, ny - 1);
        const int x0 = max(cx - r, 0), x1 = min(cx + r, nx - 1);
        for (int z = z0; z <= z1 && go_on(); ++z) {
            if (cell_start[(z * ny + y0) * nx] == cell_start[(z * ny + y1) * nx + nx]) // the empty-slab skip
                continue;
            for (int y = y0; y <= y1 && go_on(); ++y) {
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
        if (!any || cut() < lb * lb)
            break;
    }
    return seen;
}

// The walk with a fixed cut: visit(d2, v, p) for the scanned points with d2 <= r2 only.
template <class Visit>
__device__ __forceinline__ int radius_walk_at(const float4 *__restrict__ S, const int32_t *__restrict__ cell_start, const SpatialGrid &G,
                                              float qx, float qy, float qz, float r2, Visit &&visit)
{
    return ring_walk(S, cell_start, G, qx, qy, qz, [r2] { return r2; }, [&](float d2, const float4 &v, int p) {
        if constexpr (std::is_void_v<decltype(visit(d2, v, p))>) {
            if (d2 <= r2)
                visit(d2, v, p);
        } else {
            return d2 <= r2 && visit(d2, v, p);
        }
    });
}

// the same as the components kernels use it: visit(d2, id), id the point's original index
template <class Visit>
__device__ __forceinline__ int radius_walk(const float4 *__restrict__ S, const int32_t *__restrict__ cell_start, const SpatialGrid &G,
                                           float qx, float qy, float qz, float r2, Visit &&visit)
{
    return radius_walk_at(S, cell_start, G, qx, qy, qz, r2, [&](float d2, const float4 &v, int) { return visit(d2, __float_as_int(v.w)); });
}

} // namespace

} // namespace gwbp
