// spatial.hip -- exact Euclidean k-nearest-neighbour search of 3-D points on a uniform grid (the reference's knn(),
// f3dgs/utils_simple_trainer.py:141-145: sklearn NearestNeighbors on a host copy), and k_neighbor_mean, the average of a field over
// each Gaussian's neighbour list.
//
//   d2(p, q) = fmaf(dz, dz, fmaf(dy, dy, dx * dx)),  dx = p.x - q.x (fp32);   dist = sqrtf(d2) (correctly rounded)
//   idx[q, 0..k-1] = the k points of smallest d2, d2 ascending, then index ascending
//
// GRID.  Cubic cells of edge h over a box that starts at lo, nx x ny x nz cells, x fastest.  A point's cell along an axis is
//   t = floorf((x - lo) / h)   clamped to [0, n - 1]                                                              (cell_axis)
// so the border cells extend to infinity and a far floater costs no cells.  k_spatial_cell_keys writes each point's linear
// key (non-finite points: the key n_cells, which sorts last and belongs to no cell), the host sorts the keys (torch.sort,
// stable), k_spatial_build writes the points in that order as (x, y, z, original index) and cell_start[c] = the first sorted
// position whose key is >= c (a binary search per cell: every entry is written by exactly one thread, no atomics, no thread
// fills a run of empty cells).
//
// SEARCH.  One lane per query, queries in the order of their own cell keys, so that the lanes of a wave walk the same cells.
// The running top-k is LaneTopK<NearestFirst> (lane_topk.h): a sorted list in LDS, one column per lane.  The walk is ring_walk.h's,
// whose header derives the bounds and the stop rule; nothing but the cut is particular to this kernel.  No lane waits for another
// lane or workgroup: there is no barrier and no flag in the kernel.
//
// WHY THE k-TH d2 IS A VALID CUT.  The walk stops after a ring when cut() < fl(LB * LB), i.e. when every unvisited point has a
// computed d2 strictly above the list's k-th d2 so far: no such point can enter the list, and the list only improves, so the cut
// only falls.  STRICTLY, because a point at exactly the k-th d2 could tie with it and win by a smaller index.  An open list has
// k-th d2 = +inf and never stops early.
#include "gwbp_dev.h"
#include "lane_topk.h"
#include "ring_walk.h"
#include "spatial_grid.h" // SpatialGrid, finite3, cell_axis, make_grid

namespace gwbp {

namespace {

constexpr int kSpatialThreads = 128; // lanes (queries) per workgroup of the search; LDS = k * 128 * 8 B <= 32 KiB

__global__ __launch_bounds__(256) void k_spatial_cell_keys(int64_t N, const float *__restrict__ P, int64_t ldp, SpatialGrid G,
                                                           int32_t *__restrict__ keys)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N)
        return;
    const float x = P[i * ldp], y = P[i * ldp + 1], z = P[i * ldp + 2];
    int key = G.n[0] * G.n[1] * G.n[2];
    if (finite3(x, y, z))
        key = (cell_axis(z, G.lo[2], G.h, G.n[2]) * G.n[1] + cell_axis(y, G.lo[1], G.h, G.n[1])) * G.n[0] +
              cell_axis(x, G.lo[0], G.h, G.n[0]);
    keys[i] = key;
}

// thread i < N: sorted[i] = (point perm[i], its index); thread c <= n_cells: cell_start[c] = lower_bound(sorted_keys, c)
__global__ __launch_bounds__(256) void k_spatial_build(int64_t N, const float *__restrict__ P, int64_t ldp,
                                                       const int32_t *__restrict__ skeys, const int64_t *__restrict__ perm,
                                                       int64_t n_cells, float4 *__restrict__ sorted, int32_t *__restrict__ cell_start)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) {
        const int64_t g = perm[i];
        sorted[i] = make_float4(P[g * ldp], P[g * ldp + 1], P[g * ldp + 2], __int_as_float((int)g));
    }
    if (i <= n_cells) {
        int64_t a = 0, b = N; // the first position in [0, N] whose key is >= i
        while (a < b) {
            const int64_t m = (a + b) >> 1;
            if (skeys[m] < (int32_t)i)
                a = m + 1;
            else
                b = m;
        }
        cell_start[i] = (int32_t)a;
    }
}

__global__ __launch_bounds__(kSpatialThreads) void k_spatial_knn(const float4 *__restrict__ S, const int32_t *__restrict__ cell_start,
                                                                 SpatialGrid G, int64_t Q, const float *__restrict__ queries,
                                                                 int64_t ldq, const int64_t *__restrict__ order, int k,
                                                                 int32_t *__restrict__ idx, float *__restrict__ dist)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int T = kSpatialThreads;
    const int tid = threadIdx.x;
    LaneTopK<NearestFirst, T> best(smem, k, tid); // squared distances, ascending

    const int64_t slot = (int64_t)blockIdx.x * T + tid;
    if (slot >= Q)
        return; // (no barrier anywhere below)
    const int64_t g = order[slot];
    const float qx = queries[g * ldq], qy = queries[g * ldq + 1], qz = queries[g * ldq + 2];
    int32_t *oi = idx + g * k;
    float *od = dist + g * k;
    if (!finite3(qx, qy, qz)) {
        for (int j = 0; j < k; ++j) {
            oi[j] = -1;
            od[j] = __uint_as_float(0x7FC00000u);
        }
        return;
    }
    best.init();
    ring_walk(S, cell_start, G, qx, qy, qz, [&] { return best.last_key; },
              [&](float d2, const float4 &v, int) { best.offer(d2, __float_as_int(v.w)); });
    for (int j = 0; j < k; ++j) {
        const int id = best.index(j);
        oi[j] = id;
        od[j] = id < 0 ? __builtin_inff() : sqrtf(best.key(j)); // (the select keeps this loop scalar: 9 VGPRs fewer than without)
    }
}

// One wave per row g: out[g, :] = (sum over the valid j, in list order, of F[idx[g, j], :]) / (their number); lanes over
// channels, four per lane.  An index outside [0, M) is skipped; a row with none left is zero.  MT: the element type of F (a half
// row is widened as it is loaded; the sums are fp32).  OT: the element type of out (a half out is the fp32 quotient rounded once, narrow<OT>).
template <int MT, int OT, bool VEC>
__global__ __launch_bounds__(256) void k_neighbor_mean(int64_t N, int64_t M, int D, int k, const int32_t *__restrict__ idx,
                                                       const typename MapElem<MT>::raw *__restrict__ F, int64_t ldf,
                                                       typename MapElem<OT>::raw *__restrict__ out, int64_t ldo)
{
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= N)
        return;
    const int32_t *row = idx + g * k;
    for (int c0 = 0; c0 < D; c0 += 256) {
        const int c = c0 + 4 * lane;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        int nv = 0;
        for (int j = 0; j < k; ++j) {
            const int id = row[j];
            if (id < 0 || id >= M)
                continue;
            ++nv;
            const float4 v = load4t<MT, VEC>(F + (int64_t)id * ldf, c, D);
            acc.x += v.x;
            acc.y += v.y;
            acc.z += v.z;
            acc.w += v.w;
        }
        if (nv > 0) {
            const float n = (float)nv;
            acc = make_float4(acc.x / n, acc.y / n, acc.z / n, acc.w / n);
        }
        store4t<OT, VEC>(out + g * ldo, c, D, acc);
    }
}

} // namespace

int launch_spatial_cell_keys(int64_t N, const float *P, int64_t ldp, const float *lo, float h, const int32_t *dims, int32_t *keys,
                             hipStream_t s)
{
    if (N == 0)
        return GWBP_OK;
    unsigned grid;
    if (int rc = grid_of("spatial_cell_keys", N, &grid, 256))
        return rc;
    hipLaunchKernelGGL(k_spatial_cell_keys, dim3(grid), dim3(256), 0, s, N, P, ldp, make_grid(lo, h, dims), keys);
    return check_hip(hipGetLastError(), "spatial_cell_keys launch");
}

int launch_spatial_build(int64_t N, const float *P, int64_t ldp, const int32_t *skeys, const int64_t *perm, int64_t n_cells,
                         float *sorted, int32_t *cell_start, hipStream_t s)
{
    unsigned grid;
    if (int rc = grid_of("spatial_build", (N > n_cells + 1 ? N : n_cells + 1), &grid, 256))
        return rc;
    hipLaunchKernelGGL(k_spatial_build, dim3(grid), dim3(256), 0, s, N, P, ldp, skeys, perm, n_cells,
                       reinterpret_cast<float4 *>(sorted), cell_start);
    return check_hip(hipGetLastError(), "spatial_build launch");
}

int launch_spatial_knn(const float *sorted, const int32_t *cell_start, const float *lo, float h, const int32_t *dims, int64_t Q,
                       const float *queries, int64_t ldq, const int64_t *order, int k, int32_t *idx, float *dist, hipStream_t s)
{
    if (Q == 0)
        return GWBP_OK;
    unsigned grid;
    if (int rc = grid_of("spatial_knn", Q, &grid, kSpatialThreads))
        return rc;
    const size_t lds = lane_columns_bytes(k, kSpatialThreads); // <= 32 KiB: below the default limit
    hipLaunchKernelGGL(k_spatial_knn, dim3(grid), dim3(kSpatialThreads), lds, s, reinterpret_cast<const float4 *>(sorted), cell_start,
                       make_grid(lo, h, dims), Q, queries, ldq, order, k, idx, dist);
    return check_hip(hipGetLastError(), "spatial_knn launch");
}

int launch_neighbor_mean(int64_t N, int64_t M, int D, int k, const int32_t *idx, const void *F, int mt, int64_t ldf, void *out, int ot,
                         int64_t ldo, hipStream_t s)
{
    if (N == 0)
        return GWBP_OK;
    unsigned grid;
    if (int rc = grid_of("neighbor_mean", N, &grid, 4))
        return rc;
    const bool vec = field_rows_vec(F, ldf, mt) && field_rows_vec(out, ldo, ot);
    with_field_type(mt, vec, [&](auto MT, auto VEC) {
        with_map_type(ot, [&](auto OT) {
            hipLaunchKernelGGL((k_neighbor_mean<MT, OT, VEC>), dim3(grid), dim3(256), 0, s, N, M, D, k, idx, field_ptr<MT>(F), ldf,
                               out_ptr<OT>(out), ldo);
        });
    });
    return check_hip(hipGetLastError(), "neighbor_mean launch");
}

} // namespace gwbp
