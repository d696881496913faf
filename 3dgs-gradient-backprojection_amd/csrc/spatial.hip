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
// The running top-k is a sorted list in LDS, [k][threads], one column per lane.  Rings of Chebyshev radius r = 0, 1, 2, ...
// around the query's cell, clipped to the grid; within a ring every run of cells along x is one contiguous span of the sorted
// points.  No lane waits for another lane or workgroup: there is no barrier and no flag in the kernel.
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
// and LB = fl(B - fl((KH + |A|) * 2^-21)) keeps the remaining quarter for its own two roundings.  A non-positive or NaN LB
// becomes 0 ("no bound").  The margin errs towards one more ring, never towards stopping.
// From an exact |p.x - q.x| >= LB with LB a float, rounding being monotone gives |dx| = |fl(p.x - q.x)| >= LB, then
// fl(dx * dx) >= fl(LB * LB), and each fmaf adds a non-negative term before a monotone rounding: the COMPUTED d2(p, q) >= fl(LB *
// LB), whichever axis carried the bound.  The lane stops after ring r when its k-th d2 is STRICTLY below fl(LB * LB), LB the
// smallest bound over the (up to six) directions that still have cells: strictly, because a point at exactly the bound could tie
// with a smaller index.  A direction whose next ring has left the grid has no points (its bound is infinite); when all six have,
// everything has been visited.  An open list has k-th d2 = +inf and never stops early.  The trip count is at most max(nx, ny, nz).
#include "gwbp_dev.h"
#include "spatial_grid.h" // SpatialGrid, finite3, cell_axis, bound_above / bound_below, make_grid, grid_of

namespace gwbp {

namespace {

constexpr int kSpatialThreads = 128; // lanes (queries) per workgroup of the search; LDS = k * 128 * 8 B <= 32 KiB
constexpr int kNoIndex = 0x7FFFFFFF; // an empty slot of the list: orders after every point at equal distance

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
    float *ld2 = smem + tid;                                   // [k][T] squared distances, ascending
    int *lid = reinterpret_cast<int *>(smem + k * T) + tid;    // [k][T] their indices

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
    for (int j = 0; j < k; ++j) {
        ld2[j * T] = __builtin_inff();
        lid[j * T] = kNoIndex;
    }
    float kd = __builtin_inff(); // the list's last entry: the k-th best so far
    int ki = kNoIndex;

    const int nx = G.n[0], ny = G.n[1], nz = G.n[2];
    const float h = G.h;
    const int cx = cell_axis(qx, G.lo[0], h, nx), cy = cell_axis(qy, G.lo[1], h, ny), cz = cell_axis(qz, G.lo[2], h, nz);
    const float ax = qx - G.lo[0], ay = qy - G.lo[1], az = qz - G.lo[2];

    auto scan = [&](int b, int e) {
        for (int p = b; p < e; ++p) {
            const float4 v = S[p];
            const float dx = v.x - qx, dy = v.y - qy, dz = v.z - qz;
            const float d2 = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
            const int id = __float_as_int(v.w);
            if (d2 < kd || (d2 == kd && id < ki)) {
                int j = k - 1; // sorted insert: shift the entries that order after (d2, id) one down
                while (j > 0) {
                    const float pd = ld2[(j - 1) * T];
                    const int pi = lid[(j - 1) * T];
                    if (pd < d2 || (pd == d2 && pi < id))
                        break;
                    ld2[j * T] = pd;
                    lid[j * T] = pi;
                    --j;
                }
                ld2[j * T] = d2;
                lid[j * T] = id;
                kd = ld2[(k - 1) * T];
                ki = lid[(k - 1) * T];
            }
        }
    };

    const int r_max = max(nx, max(ny, nz)); // the ring has left the grid on every side by then
    for (int r = 0; r <= r_max; ++r) {
        const int z0 = max(cz - r, 0), z1 = min(cz + r, nz - 1);
        const int y0 = max(cy - r, 0), y1 = min(cy + r, ny - 1);
        const int x0 = max(cx - r, 0), x1 = min(cx + r, nx - 1);
        for (int z = z0; z <= z1; ++z) {
            // rows y0 .. y1 of this slab over the grid's full width hold everything the ring visits in it: nothing there, nothing
            // to visit (a floater in a border cell crosses the empty part of the grid in O(r) steps per ring, not O(r^2))
            if (cell_start[(z * ny + y0) * nx] == cell_start[(z * ny + y1) * nx + nx])
                continue;
            for (int y = y0; y <= y1; ++y) {
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
        if (!any || kd < lb * lb)
            break;
    }

    for (int j = 0; j < k; ++j) {
        const int id = lid[j * T];
        oi[j] = id == kNoIndex ? -1 : id;
        od[j] = id == kNoIndex ? __builtin_inff() : sqrtf(ld2[j * T]);
    }
}

// One wave per row g: out[g, :] = (sum over the valid j, in list order, of F[idx[g, j], :]) / (their number); lanes over
// channels, four per lane.  An index outside [0, M) is skipped; a row with none left is zero.  MT: the element type of F (a half
// row is widened as it is loaded; the sums and out are fp32).
template <int MT, bool VEC>
__global__ __launch_bounds__(256) void k_neighbor_mean(int64_t N, int64_t M, int D, int k, const int32_t *__restrict__ idx,
                                                       const typename MapElem<MT>::raw *__restrict__ F, int64_t ldf,
                                                       float *__restrict__ out, int64_t ldo)
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
        float *o = out + g * ldo;
        if (VEC && c + 4 <= D) {
            *reinterpret_cast<float4 *>(o + c) = acc;
        } else {
            if (c < D)
                o[c] = acc.x;
            if (c + 1 < D)
                o[c + 1] = acc.y;
            if (c + 2 < D)
                o[c + 2] = acc.z;
            if (c + 3 < D)
                o[c + 3] = acc.w;
        }
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
    const size_t lds = (size_t)k * kSpatialThreads * (sizeof(float) + sizeof(int)); // <= 32 KiB: below the default limit
    hipLaunchKernelGGL(k_spatial_knn, dim3(grid), dim3(kSpatialThreads), lds, s, reinterpret_cast<const float4 *>(sorted), cell_start,
                       make_grid(lo, h, dims), Q, queries, ldq, order, k, idx, dist);
    return check_hip(hipGetLastError(), "spatial_knn launch");
}

template <int MT>
static void launch_neighbor_mean_t(unsigned grid, hipStream_t s, int64_t N, int64_t M, int D, int k, const int32_t *idx, const void *Fv,
                                   int64_t ldf, float *out, int64_t ldo)
{
    const typename MapElem<MT>::raw *F = static_cast<const typename MapElem<MT>::raw *>(Fv);
    const bool vec = field_rows_vec(Fv, ldf, MT) && field_rows_vec(out, ldo, GWBP_MAP_F32);
    if (vec)
        hipLaunchKernelGGL((k_neighbor_mean<MT, true>), dim3(grid), dim3(256), 0, s, N, M, D, k, idx, F, ldf, out, ldo);
    else
        hipLaunchKernelGGL((k_neighbor_mean<MT, false>), dim3(grid), dim3(256), 0, s, N, M, D, k, idx, F, ldf, out, ldo);
}

int launch_neighbor_mean(int64_t N, int64_t M, int D, int k, const int32_t *idx, const void *F, int mt, int64_t ldf, float *out,
                         int64_t ldo, hipStream_t s)
{
    if (N == 0)
        return GWBP_OK;
    unsigned grid;
    if (int rc = grid_of("neighbor_mean", N, &grid, 4))
        return rc;
    if (mt == GWBP_MAP_F16)
        launch_neighbor_mean_t<GWBP_MAP_F16>(grid, s, N, M, D, k, idx, F, ldf, out, ldo);
    else if (mt == GWBP_MAP_BF16)
        launch_neighbor_mean_t<GWBP_MAP_BF16>(grid, s, N, M, D, k, idx, F, ldf, out, ldo);
    else
        launch_neighbor_mean_t<GWBP_MAP_F32>(grid, s, N, M, D, k, idx, F, ldf, out, ldo);
    return check_hip(hipGetLastError(), "neighbor_mean launch");
}

} // namespace gwbp
