// components.hip -- which points form one object: connected components of 3-D points under "within a radius of each other, and in
// the same group", as DBSCAN with a deterministic border rule (sklearn DBSCAN / Open3D cluster_dbscan / PCL Euclidean cluster
// extraction; the reference would run sklearn on a host copy, as for its only neighbour search, f3dgs/utils_simple_trainer.py:141-145).
// On the grid of spatial.hip: gwbp_spatial_cell_keys, the host's stable sort and gwbp_spatial_build make the sorted points
// (x, y, z, original index) and cell_start; spatial_grid.h holds the one cell expression and the bounds both files use.
//
//   d2(p, q) = fmaf(dz, dz, fmaf(dy, dy, dx * dx)),  dx = p.x - q.x (fp32; symmetric);   r2 = the host's fp32 radius * radius
//   live(i)      = finite coordinates and group[i] >= 0 (no group: every finite point)
//   i ~ j        = both live, group[i] == group[j], d2 <= r2            (a point is its own neighbour)
//   count[i]     = |{j : i ~ j}|;   core(i) = count[i] >= min_points
//   components   = the classes of the core points under chains of ~ through core points; a live non-core point with a core
//                  neighbour goes with its nearest core neighbour by (d2, index); everything else is noise
//
// RADIUS WALK (radius_walk of ring_walk.h: the walk of k_spatial_knn with the fixed cut r2, whose header has the bounds and the
// stop rule).  One lane per query, queries in the order of their cell keys; the lane stops after a ring when r2 < fl(LB * LB), and
// every unvisited point then has a computed d2 > r2 and is no neighbour.  STRICTLY: a point at exactly the bound may have d2 == r2,
// which counts.  The set of neighbours found is the brute-force set, whatever the grid.
//
// BORDER RULE.  A live non-core point goes with its nearest core neighbour by (d2, index): a total order on a set, so the result
// does not depend on the order in which the walk visits the neighbours.
//
// UNION-FIND BY INDEX (k_radius_union, k_components_flatten): uf_find / uf_unite of union_find.h, which regions.hip shares; the
// header has the argument.  parent[v] is the identity on entry, a hook stores a smaller index over a root, a component's final root
// is its smallest member, no lane ever waits for another, and the results do not depend on the order of the hooks.
#include "gwbp_dev.h"
#include "ring_walk.h"
#include "spatial_grid.h"
#include "union_find.h"

namespace gwbp {

namespace {

constexpr int kRadiusThreads = 128; // lanes (queries) per workgroup of a walk: two waves walking neighbouring cells

__global__ __launch_bounds__(kRadiusThreads) void k_radius_count(const float4 *__restrict__ S, const int32_t *__restrict__ cell_start,
                                                                  SpatialGrid G, const int32_t *__restrict__ group, float r2, int64_t Q,
                                                                  const float *__restrict__ queries, int64_t ldq,
                                                                  const int64_t *__restrict__ order,
                                                                  const int32_t *__restrict__ query_group, int cap,
                                                                  int32_t *__restrict__ count, int32_t *__restrict__ visited)
{
    const int64_t slot = (int64_t)blockIdx.x * kRadiusThreads + threadIdx.x;
    if (slot >= Q)
        return;
    const int64_t g = order[slot];
    const float qx = queries[g * ldq], qy = queries[g * ldq + 1], qz = queries[g * ldq + 2];
    const int qg = query_group ? query_group[g] : 0;
    int c = 0, seen = 0;
    if (finite3(qx, qy, qz) && qg >= 0)
        seen = radius_walk(S, cell_start, G, qx, qy, qz, r2, [&](float, int id) {
            if (!group || group[id] == qg)
                ++c;
            return c >= cap;
        });
    count[g] = c;
    if (visited)
        visited[g] = seen;
}

// lane = sorted position; the lanes of core points unite with their core neighbours of smaller index
__global__ __launch_bounds__(kRadiusThreads) void k_radius_union(int64_t N, const float4 *__restrict__ S,
                                                                  const int32_t *__restrict__ cell_start, SpatialGrid G,
                                                                  const int32_t *__restrict__ group, float r2,
                                                                  const int32_t *__restrict__ count, int min_points, int32_t *parent,
                                                                  int32_t *status)
{
    const int64_t slot = (int64_t)blockIdx.x * kRadiusThreads + threadIdx.x;
    if (slot >= N)
        return;
    const float4 v = S[slot];
    const int i = __float_as_int(v.w);
    if (!finite3(v.x, v.y, v.z) || count[i] < min_points) // (count is 0 for a point that is not live)
        return;
    const int gi = group ? group[i] : 0;
    const int cap = (int)min(N + 1, (int64_t)0x7FFFFFFF);
    int mine = i; // an ancestor of i: where the next find starts
    radius_walk(S, cell_start, G, v.x, v.y, v.z, r2, [&](float, int j) {
        if (j < i && count[j] >= min_points && (!group || group[j] == gi))
            mine = uf_unite(parent, mine, j, cap, status);
    });
}

// lane = sorted position; a live non-core point's nearest core neighbour by (d2, index)
__global__ __launch_bounds__(kRadiusThreads) void k_radius_attach(int64_t N, const float4 *__restrict__ S,
                                                                   const int32_t *__restrict__ cell_start, SpatialGrid G,
                                                                   const int32_t *__restrict__ group, float r2,
                                                                   const int32_t *__restrict__ count, int min_points,
                                                                   int32_t *__restrict__ attach)
{
    const int64_t slot = (int64_t)blockIdx.x * kRadiusThreads + threadIdx.x;
    if (slot >= N)
        return;
    const float4 v = S[slot];
    const int i = __float_as_int(v.w);
    int best = -1;
    if (finite3(v.x, v.y, v.z) && count[i] > 0 && count[i] < min_points) {
        const int gi = group ? group[i] : 0;
        float bd = __builtin_inff();
        radius_walk(S, cell_start, G, v.x, v.y, v.z, r2, [&](float d2, int j) {
            if (count[j] >= min_points && (!group || group[j] == gi) && (best < 0 || d2 < bd || (d2 == bd && j < best))) {
                bd = d2;
                best = j;
            }
        });
    }
    attach[i] = best;
}

__global__ __launch_bounds__(256) void k_components_flatten(int64_t N, const int32_t *__restrict__ count, int min_points,
                                                            const int32_t *__restrict__ attach, int32_t *parent,
                                                            int32_t *__restrict__ root, int32_t *status)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N)
        return;
    const int cap = (int)min(N + 1, (int64_t)0x7FFFFFFF);
    int from = -1;
    if (count[i] >= min_points)
        from = (int)i;
    else if (attach)
        from = attach[i];
    root[i] = from >= 0 ? uf_find(parent, from, cap, status) : -1;
}

} // namespace

int launch_radius_count(const float *sorted, const int32_t *cell_start, const float *lo, float h, const int32_t *dims,
                        const int32_t *group, float r2, int64_t Q, const float *queries, int64_t ldq, const int64_t *order,
                        const int32_t *query_group, int cap, int32_t *count, int32_t *visited, hipStream_t s)
{
    if (Q == 0)
        return GWBP_OK;
    unsigned grid;
    if (int rc = grid_of("radius_count", Q, &grid, kRadiusThreads))
        return rc;
    hipLaunchKernelGGL(k_radius_count, dim3(grid), dim3(kRadiusThreads), 0, s, reinterpret_cast<const float4 *>(sorted), cell_start,
                       make_grid(lo, h, dims), group, r2, Q, queries, ldq, order, query_group, cap, count, visited);
    return check_hip(hipGetLastError(), "radius_count launch");
}

int launch_radius_union(int64_t N, const float *sorted, const int32_t *cell_start, const float *lo, float h, const int32_t *dims,
                        const int32_t *group, float r2, const int32_t *count, int min_points, int32_t *parent, int32_t *status,
                        hipStream_t s)
{
    unsigned grid;
    if (int rc = grid_of("radius_union", N, &grid, kRadiusThreads))
        return rc;
    hipLaunchKernelGGL(k_radius_union, dim3(grid), dim3(kRadiusThreads), 0, s, N, reinterpret_cast<const float4 *>(sorted), cell_start,
                       make_grid(lo, h, dims), group, r2, count, min_points, parent, status);
    return check_hip(hipGetLastError(), "radius_union launch");
}

int launch_radius_attach(int64_t N, const float *sorted, const int32_t *cell_start, const float *lo, float h, const int32_t *dims,
                         const int32_t *group, float r2, const int32_t *count, int min_points, int32_t *attach, hipStream_t s)
{
    unsigned grid;
    if (int rc = grid_of("radius_attach", N, &grid, kRadiusThreads))
        return rc;
    hipLaunchKernelGGL(k_radius_attach, dim3(grid), dim3(kRadiusThreads), 0, s, N, reinterpret_cast<const float4 *>(sorted), cell_start,
                       make_grid(lo, h, dims), group, r2, count, min_points, attach);
    return check_hip(hipGetLastError(), "radius_attach launch");
}

int launch_components_flatten(int64_t N, const int32_t *count, int min_points, const int32_t *attach, int32_t *parent, int32_t *root,
                              int32_t *status, hipStream_t s)
{
    unsigned grid;
    if (int rc = grid_of("components_flatten", N, &grid, 256))
        return rc;
    hipLaunchKernelGGL(k_components_flatten, dim3(grid), dim3(256), 0, s, N, count, min_points, attach, parent, root, status);
    return check_hip(hipGetLastError(), "components_flatten launch");
}

} // namespace gwbp
