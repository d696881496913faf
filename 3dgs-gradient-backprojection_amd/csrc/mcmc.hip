// mcmc.hip -- gsplat's MCMCStrategy on a set of Gaussians during training: dead Gaussians move onto alive ones drawn
// by opacity, the set grows by 5 % a round up to a cap, and every step adds opacity-gated noise to the means.  mcmc_math.h carries every
// expression that is not a memory access.
//
//   k_mcmc_plan       a lane per Gaussian: the integer weight floor(sigmoid(opacity) 2^24) (0 for a dead one in relocate mode) and the
//                     dead flag; the workgroup's exclusive scans of both go to cdf and dead_offsets, the totals to the two halves of sums.
//   k_scan_block_sums (block_scan.h, shared with densify.hip) once per half: sums becomes its own exclusive scan, cdf[N] and
//                     dead_offsets[N] the grand totals.
//   k_mcmc_plan_add   cdf[i] += wsum[i / 256], dead_offsets[i] += dsum[i / 256], and the compaction dead_idx[dead_offsets[i]] = i.
//   k_mcmc_draw       a lane per draw j: t = min((int64)(u[j] total), total - 1); parent[j] = the i with cdf[i] <= t < cdf[i + 1] by
//                     binary search.  u ascending gives parent ascending.
//   k_mcmc_update     a lane per Gaussian: count[i] = the number of j with parent[j] == i, by two binary searches in the ascending
//                     parent; where it is positive the row's opacity and scaling become mcmc_relocate(.., min(count + 1, 51)) IN PLACE.
//   k_mcmc_move       table[dead_idx[j], :] = table[parent[j], :] IN PLACE, lanes along the rows of a workgroup's RB consecutive j.  A dead
//                     row has weight 0 and is never a parent, so no row is both read and written.
//   k_mcmc_zero_rows  table[i, :] = 0 where count[i] > 0.
//   k_mcmc_noise      (every training step) a lane per Gaussian: means[i] = mcmc_noise(...), in place.
//   k_mcmc_libm       out = expf(a) | logf(a) | powf(a, b), elementwise: the device's library under this build's flags, for the tests
//                     that hold the kernels to the numpy restatement bit for bit.
//
// No atomics and no waits between workgroups: integer sums in a fixed order, the same bits for the same inputs.  Every loop bound is a
// kernel argument.  Every store is a vector store.  A row index is checked against its array before anything is written through it: a
// parent or dead_idx outside [0, n) moves nothing, a parent array that is not ascending gives wrong counts and no write out of bounds.
#include "gwbp_dev.h"
#include "block_scan.h"
#include "mcmc_math.h"

namespace gwbp {

namespace {

constexpr int kBlock = GWBP_DENSIFY_BLOCK;
constexpr int kMoveMaxRows = GWBP_DENSIFY_GATHER_MAX_ROWS;

__global__ __launch_bounds__(256) void k_mcmc_plan(int64_t N, const float *__restrict__ opacity, float t_opa, float t_weight,
                                                   int64_t *__restrict__ cdf, int64_t *__restrict__ dead_offsets,
                                                   int64_t *__restrict__ wsum, int64_t *__restrict__ dsum)
{
    __shared__ long long wave_w[4], wave_d[4];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    long long w = 0, d = 0;
    if (i < N) {
        const float o = opacity[i];
        w = mcmc_weight(o, t_weight);
        d = !(o > t_opa);
    }
    long long tw, td;
    const long long bw = block_exclusive<long long>(w, wave_w, &tw);
    const long long bd = block_exclusive<long long>(d, wave_d, &td);
    if (i < N)
        cdf[i] = bw, dead_offsets[i] = bd;
    if (threadIdx.x == 0)
        wsum[blockIdx.x] = tw, dsum[blockIdx.x] = td;
}

__global__ __launch_bounds__(256) void k_mcmc_plan_add(int64_t N, const float *__restrict__ opacity, float t_opa,
                                                       const int64_t *__restrict__ wsum, const int64_t *__restrict__ dsum,
                                                       int64_t *__restrict__ cdf, int64_t *__restrict__ dead_offsets, int32_t *__restrict__ dead_idx)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= N)
        return;
    cdf[i] += wsum[blockIdx.x];
    const int64_t at = dead_offsets[i] + dsum[blockIdx.x];
    dead_offsets[i] = at;
    if (!(opacity[i] > t_opa) && at >= 0 && at < N)
        dead_idx[at] = (int32_t)i;
}

__global__ __launch_bounds__(256) void k_mcmc_draw(int64_t N, int64_t M, const int64_t *__restrict__ cdf, const double *__restrict__ u,
                                                   int32_t *__restrict__ parent)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= M)
        return;
    const int64_t total = cdf[N];
    if (total <= 0) {
        parent[j] = -1;
        return;
    }
    const double x = u[j] * (double)total;
    int64_t t = x >= (double)total ? total - 1 : x > 0.0 ? (int64_t)x : 0; // (a NaN draws the first alive Gaussian)
    t = t < total - 1 ? t : total - 1;
    int64_t lo = 0, hi = N - 1; // the last i with cdf[i] <= t: cdf[0] = 0 <= t, and t < cdf[N]
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (cdf[mid] <= t)
            lo = mid;
        else
            hi = mid - 1;
    }
    parent[j] = (int32_t)lo;
}

// the first j in [0, M) with parent[j] >= key (M if none)
__device__ __forceinline__ int64_t lower_bound_i32(const int32_t *__restrict__ a, int64_t M, int64_t key)
{
    int64_t lo = 0, hi = M;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)a[mid] < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_mcmc_update(int64_t N, int64_t M, const int32_t *__restrict__ parent, float min_opacity,
                                                     float *__restrict__ opacity, float *__restrict__ scaling, int64_t lds_,
                                                     int32_t *__restrict__ count)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= N)
        return;
    const int64_t first = lower_bound_i32(parent, M, i), last = lower_bound_i32(parent, M, i + 1);
    const int64_t c = last > first ? last - first : 0;
    count[i] = (int32_t)c;
    if (c == 0)
        return;
    const int ratio = c + 1 < kMcmcMaxRatio ? (int)(c + 1) : kMcmcMaxRatio;
    float *s = scaling + i * lds_;
    const float s3[3] = {s[0], s[1], s[2]};
    float o, so[3];
    mcmc_relocate(opacity[i], s3, ratio, min_opacity, &o, so);
    opacity[i] = o;
    s[0] = so[0], s[1] = so[1], s[2] = so[2];
}

__global__ __launch_bounds__(256) void k_mcmc_move(int64_t N, int64_t M, int w, int rb, const int32_t *__restrict__ parent,
                                                   const int32_t *__restrict__ dead_idx, float *table, int64_t ldt)
{
    __shared__ int32_t src[kMoveMaxRows], dst[kMoveMaxRows]; // -1: nothing moves
    const int64_t j0 = (int64_t)blockIdx.x * rb;
    const int rows = (int)min((int64_t)rb, M - j0);
    for (int j = threadIdx.x; j < rows; j += kBlock) {
        int32_t p = parent[j0 + j], d = dead_idx[j0 + j];
        if (p < 0 || (int64_t)p >= N || d < 0 || (int64_t)d >= N || p == d)
            p = -1, d = -1;
        src[j] = p, dst[j] = d;
    }
    __syncthreads();
    const unsigned total = (unsigned)rows * (unsigned)w;
    for (unsigned e = threadIdx.x; e < total; e += kBlock) {
        const unsigned j = e / (unsigned)w, c = e - j * (unsigned)w;
        const int32_t p = src[j];
        if (p >= 0)
            table[(int64_t)dst[j] * ldt + c] = table[(int64_t)p * ldt + c];
    }
}

__global__ __launch_bounds__(256) void k_mcmc_zero_rows(int64_t N, int w, int rb, const int32_t *__restrict__ count, float *__restrict__ table,
                                                        int64_t ldt)
{
    __shared__ uint8_t hit[kMoveMaxRows];
    const int64_t r0 = (int64_t)blockIdx.x * rb;
    const int rows = (int)min((int64_t)rb, N - r0);
    for (int j = threadIdx.x; j < rows; j += kBlock)
        hit[j] = count[r0 + j] > 0;
    __syncthreads();
    const unsigned total = (unsigned)rows * (unsigned)w;
    for (unsigned e = threadIdx.x; e < total; e += kBlock) {
        const unsigned j = e / (unsigned)w, c = e - j * (unsigned)w;
        if (hit[j])
            table[(r0 + j) * ldt + c] = 0.0f;
    }
}

__global__ __launch_bounds__(256) void k_mcmc_noise(int64_t N, float *__restrict__ means, const float *__restrict__ scaling,
                                                    const float *__restrict__ rotation, const float *__restrict__ opacity,
                                                    const float *__restrict__ z, float scaler)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= N)
        return;
    float m[3], s[3], q[4], z3[3], out[3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
        m[j] = means[i * 3 + j], s[j] = scaling[i * 3 + j], z3[j] = z[i * 3 + j];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        q[j] = rotation[i * 4 + j];
    mcmc_noise(m, s, q, opacity[i], z3, scaler, out);
#pragma unroll
    for (int j = 0; j < 3; ++j)
        means[i * 3 + j] = out[j];
}

__global__ __launch_bounds__(256) void k_mcmc_libm(int64_t N, int op, const float *__restrict__ a, const float *__restrict__ b,
                                                   float *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= N)
        return;
    out[i] = op == GWBP_MCMC_LIBM_EXP ? expf(a[i]) : op == GWBP_MCMC_LIBM_LOG ? logf(a[i]) : powf(a[i], b[i]);
}

// rows per workgroup of the row-tiled kernels: about 4096 elements, between 16 and kMoveMaxRows rows
int rows_per_block(int w)
{
    const int rb = 4096 / w;
    return rb < 16 ? 16 : rb > kMoveMaxRows ? kMoveMaxRows : rb;
}

} // namespace

size_t mcmc_plan_workspace_bytes(int64_t n)
{
    const int64_t blocks = (n + kBlock - 1) / kBlock;
    return (size_t)(blocks > 0 ? blocks : 1) * 2 * sizeof(int64_t);
}

int launch_mcmc_plan(int64_t N, const float *opacity, float t_opa, int add_mode, int64_t *cdf, int64_t *dead_offsets, int32_t *dead_idx,
                     void *ws, hipStream_t s)
{
    unsigned grid;
    if (int rc = grid_of("mcmc_plan", N, &grid, kBlock))
        return rc;
    int64_t *wsum = static_cast<int64_t *>(ws), *dsum = wsum + (grid > 0 ? grid : 1);
    const float t_weight = add_mode ? -INFINITY : t_opa;
    if (grid > 0)
        hipLaunchKernelGGL(k_mcmc_plan, dim3(grid), dim3(kBlock), 0, s, N, opacity, t_opa, t_weight, cdf, dead_offsets, wsum, dsum);
    hipLaunchKernelGGL(k_scan_block_sums, dim3(1), dim3(kBlock), 0, s, (int64_t)grid, wsum, cdf + N);
    hipLaunchKernelGGL(k_scan_block_sums, dim3(1), dim3(kBlock), 0, s, (int64_t)grid, dsum, dead_offsets + N);
    if (grid > 0)
        hipLaunchKernelGGL(k_mcmc_plan_add, dim3(grid), dim3(kBlock), 0, s, N, opacity, t_opa, wsum, dsum, cdf, dead_offsets, dead_idx);
    return check_hip(hipGetLastError(), "mcmc_plan launch");
}

int launch_mcmc_draw(int64_t N, int64_t M, const int64_t *cdf, const double *u, int32_t *parent, hipStream_t s)
{
    unsigned grid;
    if (int rc = grid_of("mcmc_draw", M, &grid, kBlock))
        return rc;
    if (grid == 0 || N == 0)
        return GWBP_OK;
    hipLaunchKernelGGL(k_mcmc_draw, dim3(grid), dim3(kBlock), 0, s, N, M, cdf, u, parent);
    return check_hip(hipGetLastError(), "mcmc_draw launch");
}

int launch_mcmc_update(int64_t N, int64_t M, const int32_t *parent, float min_opacity, float *opacity, float *scaling, int64_t lds_,
                       int32_t *count, hipStream_t s)
{
    unsigned grid;
    if (int rc = grid_of("mcmc_update", N, &grid, kBlock))
        return rc;
    if (grid == 0)
        return GWBP_OK;
    hipLaunchKernelGGL(k_mcmc_update, dim3(grid), dim3(kBlock), 0, s, N, M, parent, min_opacity, opacity, scaling, lds_, count);
    return check_hip(hipGetLastError(), "mcmc_update launch");
}

int launch_mcmc_move(int64_t N, int64_t M, int w, const int32_t *parent, const int32_t *dead_idx, float *table, int64_t ldt, hipStream_t s)
{
    if (N == 0 || M == 0)
        return GWBP_OK;
    const int rb = rows_per_block(w);
    unsigned grid;
    if (int rc = grid_of("mcmc_move", M, &grid, rb))
        return rc;
    hipLaunchKernelGGL(k_mcmc_move, dim3(grid), dim3(kBlock), 0, s, N, M, w, rb, parent, dead_idx, table, ldt);
    return check_hip(hipGetLastError(), "mcmc_move launch");
}

int launch_mcmc_zero_rows(int64_t N, int w, const int32_t *count, float *table, int64_t ldt, hipStream_t s)
{
    if (N == 0)
        return GWBP_OK;
    const int rb = rows_per_block(w);
    unsigned grid;
    if (int rc = grid_of("mcmc_zero_rows", N, &grid, rb))
        return rc;
    hipLaunchKernelGGL(k_mcmc_zero_rows, dim3(grid), dim3(kBlock), 0, s, N, w, rb, count, table, ldt);
    return check_hip(hipGetLastError(), "mcmc_zero_rows launch");
}

int launch_mcmc_noise(int64_t N, float *means, const float *scaling, const float *rotation, const float *opacity, const float *z,
                      float scaler, hipStream_t s)
{
    unsigned grid;
    if (int rc = grid_of("mcmc_noise", N, &grid, kBlock))
        return rc;
    if (grid == 0)
        return GWBP_OK;
    hipLaunchKernelGGL(k_mcmc_noise, dim3(grid), dim3(kBlock), 0, s, N, means, scaling, rotation, opacity, z, scaler);
    return check_hip(hipGetLastError(), "mcmc_noise launch");
}

int launch_mcmc_libm(int64_t N, int op, const float *a, const float *b, float *out, hipStream_t s)
{
    unsigned grid;
    if (int rc = grid_of("mcmc_libm", N, &grid, kBlock))
        return rc;
    if (grid == 0)
        return GWBP_OK;
    hipLaunchKernelGGL(k_mcmc_libm, dim3(grid), dim3(kBlock), 0, s, N, op, a, b, out);
    return check_hip(hipGetLastError(), "mcmc_libm launch");
}

} // namespace gwbp
