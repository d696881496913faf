// densify.hip -- growing and pruning a set of Gaussians during training (gsplat's DefaultStrategy): the per-step
// statistics, the rule, and the relocation of every per-Gaussian table.  densify_math.h carries every expression that is not a memory
// access.
//
//   k_densify_accumulate  a lane per Gaussian, the cameras one after the other: grad2d += |(gx sx, gy sy)|, count += 1 where the row is
//                         visible.  One pass over [C, N, 2] + [C, N]; the per-step hot path.
//   k_densify_plan        a lane per Gaussian: kind (pruned, keep, clone, split) and rows out (0, 1, 2, 2); the workgroup's exclusive scan
//                         of the rows (wave scan by shuffles, the four wave totals through LDS) goes to offsets, its total to sums[block].
//   k_scan_block_sums     (block_scan.h, shared with mcmc.hip) ONE workgroup walks sums in chunks of 256 in ascending order with a
//                         running carry: sums becomes its own exclusive scan, offsets[N] the grand total.
//   k_densify_add         offsets[i] += sums[i / 256].
//   k_densify_emit        a lane per parent: its 0, 1 or 2 children at offsets[p], in parent order.
//   k_densify_gather      out[r, :] = table[parent[r], :], lanes along the rows of a workgroup's RB consecutive output rows (the RB
//                         parents and zero flags pass through LDS): the writes of a dense output are one contiguous run, the reads
//                         contiguous inside a row.
//
// No atomics and no waits between workgroups: integer sums in a fixed order, the same bits for the same inputs.  Every loop bound is a
// kernel argument.  Every store is a vector store.  A row index is checked against its array before anything is written through it: an
// offsets array that does not belong to n_out, or a parent outside [0, n), writes nothing out of bounds (emit drops the row, gather writes
// a zero row).
#include "gwbp_dev.h"
#include "block_scan.h"
#include "densify_math.h"

namespace gwbp {

namespace {

constexpr int kBlock = GWBP_DENSIFY_BLOCK;
static_assert(kBlock == 256, "the scans below are written for four waves of 64");

__global__ __launch_bounds__(256) void k_densify_accumulate(int64_t N, int C, const float2 *__restrict__ v, const int32_t *__restrict__ radii,
                                                            float sx, float sy, float *__restrict__ grad2d, float *__restrict__ count)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= N)
        return;
    float g = grad2d[i], n = count[i];
    for (int c = 0; c < C; ++c) {
        const int64_t at = (int64_t)c * N + i;
        if (radii[at] > 0) {
            const float2 d = v[at];
            g += densify_norm(d.x, d.y, sx, sy);
            n += 1.0f;
        }
    }
    grad2d[i] = g, count[i] = n;
}

__global__ __launch_bounds__(256) void k_densify_plan(int64_t N, const float *__restrict__ grad2d, const float *__restrict__ count,
                                                      const float *__restrict__ scaling, int64_t lds_, const float *__restrict__ opacity,
                                                      DensifyThresholds T, uint8_t *__restrict__ kind, int64_t *__restrict__ offsets,
                                                      int64_t *__restrict__ sums)
{
    __shared__ int wave_tot[4];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int k = kDensifyPruned, rows = 0;
    if (i < N) {
        const float *s = scaling + i * lds_;
        k = densify_kind(grad2d[i], count[i], s[0], s[1], s[2], opacity[i], T);
        rows = densify_rows(k);
        kind[i] = (uint8_t)k;
    }
    int total;
    const int before = block_exclusive<int>(rows, wave_tot, &total);
    if (i < N)
        offsets[i] = before;
    if (threadIdx.x == 0)
        sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_densify_add(int64_t N, const int64_t *__restrict__ sums, int64_t *__restrict__ offsets)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < N)
        offsets[i] += sums[blockIdx.x];
}

struct EmitArgs { // wave-uniform
    const float *means, *scaling, *rotation, *opacity, *noise;
    int32_t *parent;
    uint8_t *child;
    float *o_means, *o_scaling, *o_rotation, *o_opacity;
};

__global__ __launch_bounds__(256) void k_densify_emit(int64_t N, int64_t n_out, const uint8_t *__restrict__ kind,
                                                      const int64_t *__restrict__ offsets, float log16, EmitArgs A)
{
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= N)
        return;
    const int k = kind[p];
    const int rows = densify_rows(k);
    const int64_t at = offsets[p];
    if (rows == 0 || at < 0)
        return;
    float m[3], s[3], q[4];
#pragma unroll
    for (int j = 0; j < 3; ++j)
        m[j] = A.means[p * 3 + j], s[j] = A.scaling[p * 3 + j];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        q[j] = A.rotation[p * 4 + j];
    const float o = A.opacity[p];
    for (int c = 0; c < rows; ++c) {
        const int64_t r = at + c;
        if (r >= n_out)
            return;
        float mo[3] = {m[0], m[1], m[2]}, so[3] = {s[0], s[1], s[2]};
        if (k == kDensifySplit) {
            const float *nz = A.noise + (p * 2 + c) * 3;
            const float z3[3] = {nz[0], nz[1], nz[2]};
            densify_split(m, s, q, z3, mo);
#pragma unroll
            for (int j = 0; j < 3; ++j)
                so[j] = s[j] - log16;
        }
        A.parent[r] = (int32_t)p;
        A.child[r] = (uint8_t)c;
#pragma unroll
        for (int j = 0; j < 3; ++j)
            A.o_means[r * 3 + j] = mo[j], A.o_scaling[r * 3 + j] = so[j];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            A.o_rotation[r * 4 + j] = q[j];
        A.o_opacity[r] = o;
    }
}

constexpr int kGatherMaxRows = GWBP_DENSIFY_GATHER_MAX_ROWS;

__global__ __launch_bounds__(256) void k_densify_gather(int64_t N, int64_t n_out, int w, int rb, const float *__restrict__ table, int64_t ldt,
                                                        const int32_t *__restrict__ parent, const uint8_t *__restrict__ child,
                                                        const uint8_t *__restrict__ kind, int zero_new, float *__restrict__ out, int64_t ldo)
{
    __shared__ int32_t src[kGatherMaxRows]; // the parent of each of the workgroup's rows, -1: a zero row
    const int64_t r0 = (int64_t)blockIdx.x * rb;
    const int rows = (int)min((int64_t)rb, n_out - r0);
    for (int j = threadIdx.x; j < rows; j += kBlock) {
        int32_t p = parent[r0 + j];
        if (p < 0 || (int64_t)p >= N)
            p = -1;
        else if (zero_new) {
            const int k = kind[p];
            if (k == kDensifySplit || (k == kDensifyClone && child[r0 + j] != 0))
                p = -1;
        }
        src[j] = p;
    }
    __syncthreads();
    const unsigned total = (unsigned)rows * (unsigned)w;
    for (unsigned e = threadIdx.x; e < total; e += kBlock) {
        const unsigned j = e / (unsigned)w, c = e - j * (unsigned)w;
        const int32_t p = src[j];
        out[(r0 + j) * ldo + c] = p < 0 ? 0.0f : table[(int64_t)p * ldt + c];
    }
}

} // namespace

int64_t densify_blocks(int64_t n) { return (n + kBlock - 1) / kBlock; }

size_t densify_plan_workspace_bytes(int64_t n) { return (size_t)(densify_blocks(n) > 0 ? densify_blocks(n) : 1) * sizeof(int64_t); }

int launch_densify_accumulate(int64_t N, int C, const float *v, const int32_t *radii, float sx, float sy, float *grad2d, float *count,
                              hipStream_t s)
{
    unsigned grid;
    if (int rc = grid_of("densify_accumulate", N, &grid, kBlock))
        return rc;
    if (grid == 0)
        return GWBP_OK;
    hipLaunchKernelGGL(k_densify_accumulate, dim3(grid), dim3(kBlock), 0, s, N, C, reinterpret_cast<const float2 *>(v), radii, sx, sy, grad2d,
                       count);
    return check_hip(hipGetLastError(), "densify_accumulate launch");
}

int launch_densify_plan(int64_t N, const float *grad2d, const float *count, const float *scaling, int64_t lds_, const float *opacity,
                        const float *thresholds, int prune_big, uint8_t *kind, int64_t *offsets, void *ws, hipStream_t s)
{
    unsigned grid;
    if (int rc = grid_of("densify_plan", N, &grid, kBlock))
        return rc;
    int64_t *sums = static_cast<int64_t *>(ws);
    DensifyThresholds T;
    T.t_grad = thresholds[0], T.t_small = thresholds[1], T.t_big = thresholds[2], T.t_opa = thresholds[3], T.log16 = thresholds[4];
    T.prune_big = prune_big != 0;
    if (grid > 0)
        hipLaunchKernelGGL(k_densify_plan, dim3(grid), dim3(kBlock), 0, s, N, grad2d, count, scaling, lds_, opacity, T, kind, offsets, sums);
    hipLaunchKernelGGL(k_scan_block_sums, dim3(1), dim3(kBlock), 0, s, (int64_t)grid, sums, offsets + N);
    if (grid > 0)
        hipLaunchKernelGGL(k_densify_add, dim3(grid), dim3(kBlock), 0, s, N, sums, offsets);
    return check_hip(hipGetLastError(), "densify_plan launch");
}

int launch_densify_emit(int64_t N, int64_t n_out, const uint8_t *kind, const int64_t *offsets, const float *means, const float *scaling,
                        const float *rotation, const float *opacity, const float *noise, float log16, int32_t *parent, uint8_t *child,
                        float *o_means, float *o_scaling, float *o_rotation, float *o_opacity, hipStream_t s)
{
    unsigned grid;
    if (int rc = grid_of("densify_emit", N, &grid, kBlock))
        return rc;
    if (grid == 0 || n_out == 0)
        return GWBP_OK;
    EmitArgs A;
    A.means = means, A.scaling = scaling, A.rotation = rotation, A.opacity = opacity, A.noise = noise;
    A.parent = parent, A.child = child;
    A.o_means = o_means, A.o_scaling = o_scaling, A.o_rotation = o_rotation, A.o_opacity = o_opacity;
    hipLaunchKernelGGL(k_densify_emit, dim3(grid), dim3(kBlock), 0, s, N, n_out, kind, offsets, log16, A);
    return check_hip(hipGetLastError(), "densify_emit launch");
}

int launch_densify_gather(int64_t N, int64_t n_out, int w, const float *table, int64_t ldt, const int32_t *parent, const uint8_t *child,
                          const uint8_t *kind, int zero_new, float *out, int64_t ldo, hipStream_t s)
{
    if (n_out == 0)
        return GWBP_OK;
    // rows per workgroup: about 4096 elements, between 16 and kGatherMaxRows rows (rows x w stays below 2^31: w <= GWBP_DENSIFY_MAX_WIDTH)
    int rb = 4096 / w;
    rb = rb < 16 ? 16 : rb > kGatherMaxRows ? kGatherMaxRows : rb;
    unsigned grid;
    if (int rc = grid_of("densify_gather", n_out, &grid, rb))
        return rc;
    hipLaunchKernelGGL(k_densify_gather, dim3(grid), dim3(kBlock), 0, s, N, n_out, w, rb, table, ldt, parent, child, kind, zero_new, out, ldo);
    return check_hip(hipGetLastError(), "densify_gather launch");
}

} // namespace gwbp
