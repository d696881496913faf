// regions.hip -- which Gaussians form one object by geometry AND features: region growing on the cosine of a feature field over a
// neighbour list (the spatial k-NN graph of spatial.hip).  k_neighbor_similarity turns "neighbour list + field" into the cosine of
// every listed pair; k_edge_union joins the pairs that pass a threshold with the union-find of union_find.h; components.hip's
// k_components_flatten reads the roots.  The kernels are split so that a sweep over thresholds pays the [N, D] pass once and only
// the integer kernel per threshold.  (The reference has nothing of the kind; its users would run a host-side graph library on a copy
// of the [N, D] field.)
//
// THE CONTRACT (include/gwbp.h, DESIGN 4.0c and tests/regions_ref.py say the same).
//   features[N, D] fp32, row stride ldf >= D;  idx[N, k] int32: an entry < 0 or >= N is no neighbour, an entry == i is allowed and
//   ignored by the union;  dist[N, k] (optional): spatial_knn's distances;  group[N] (optional) int32.
//   dot(i, j) = sum_c F[i, c] F[j, c] and sq(i) = dot(i, i): lane l of the wave owns the channels 256 s + 4 l + e (s = 0, 1, ...;
//     e = 0 .. 3; those < D) and runs acc = fmaf(a, b, acc) from acc = +0 in the order (s, e); the 64 partial sums are combined by the
//     butterfly p_l = p_l + p_(l xor o), o = 1, 2, 4, 8, 16, 32.  A channel >= D enters as a product of zeros, which leaves the
//     bits as skipping it would: an accumulator that starts at +0 never becomes -0.  The arrangement depends on D alone.
//     It is SYMMETRIC: fmaf(a, b, .) == fmaf(b, a, .) and x + y == y + x bit for bit, so dot(i, j) computed in row i's wave has the
//     bits of dot(j, i) computed in row j's, and sq(j) is the same chain over the same registers whichever wave loaded them.  It is
//     independent of N, k, the row's position, ldf, the alignment (the 16-B and the element-wise loads fill the same registers) and
//     the launch.  (wave_sum of gwbp_dev.h IS that butterfly: after the four DPP steps the 16 lanes of a row hold one value, and
//     (r0 + r1) + (r2 + r3) is what every lane of the steps o = 16, 32 computes, up to the order of the operands of an addition.)
//   norm(i) = sqrtf(sq(i)), correctly rounded;  FEATURE-LIVE(i) = sq(i) finite and norm(i) >= 1e-12f (F.normalize's epsilon);
//   sim[i, c] = dot(i, j) / (norm(i) * norm(j)), j = idx[i, c]: one multiply, one correctly rounded divide (query.hip's); NaN when j is
//     no neighbour or either row is not feature-live;
//   live(i) = feature-live and group[i] >= 0 (no group: 0);
//   i -- j is an EDGE when j = idx[i, c] for some c or i = idx[j, c], i != j, both live, group[i] == group[j], sim[i, c] >= sim_min
//     (NaN fails), and, when a cut is given (dist and max_dist < +inf), dist[i, c] <= max_dist;
//   labels = the connected components of the live points under the edges; root = the smallest member; everything else -1.
//
// k_neighbor_similarity: one wave per row i, four waves per workgroup, the shape of k_neighbor_mean.  Row i sits in registers (NS
// float4 per lane, NS = 1, 2, 4 or 8 steps of 256 channels: D <= 2048); the neighbour rows arrive two at a time, all loads of both
// issued before the first use, with 16-B loads when address and stride allow (load4<VEC>), else element by element.  For each
// neighbour the wave runs both chains on the loaded registers (dot, and the neighbour's sq), the two reductions, the sqrt and the
// divide; lane 0 stores.  Every loop bound is wave-uniform (k, NS; the neighbour's index is read through readfirstlane); no atomics,
// no LDS, no inter-wave communication.  A gather-bound kernel: (k + 1) N rows of 4 D bytes, about 2 FLOP per 4 bytes; no MFMA work.
//
// k_edge_union: one lane per row i over its k entries: the edge test above and uf_unite(i, j).  sim[i, c] is not NaN only when
// both rows are feature-live, so the lane reads no live[j]; it reads group[j].  An edge listed from one side only joins the two
// all the same (unite is symmetric), and one listed from both sides is united twice, which changes nothing.  No lane waits for
// another lane's write; the labels are the transitive closure of the united pairs, whatever the order (union_find.h).
#include "gwbp_dev.h"
#include "union_find.h"

namespace gwbp {

namespace {

constexpr int kUnionThreads = 128;

// one lane's chain over its channels, order (s, e), from +0
template <int NS>
__device__ __forceinline__ float lane_chain(const float4 (&a)[NS], const float4 (&b)[NS])
{
    float acc = 0.0f;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        acc = __builtin_fmaf(a[s].x, b[s].x, acc);
        acc = __builtin_fmaf(a[s].y, b[s].y, acc);
        acc = __builtin_fmaf(a[s].z, b[s].z, acc);
        acc = __builtin_fmaf(a[s].w, b[s].w, acc);
    }
    return acc;
}

// MT: the element type of the field.  load_row lands a row's bits (zeros beyond D and for p == nullptr, without a load); widen_row
// turns them into the registers the fp32 kernel's loads fill (exact; fp32: the identity) once every load of the step is issued.
template <int MT, bool VEC, int NS>
__device__ __forceinline__ void load_row(typename MapElem<MT>::raw4 (&r)[NS], const void *__restrict__ p, int lane, int D)
{
#pragma unroll
    for (int s = 0; s < NS; ++s)
        r[s] = load4raw<MT, VEC>(p, 256 * s + 4 * lane, D);
}
template <int MT, int NS>
__device__ __forceinline__ void widen_row(float4 (&x)[NS], const typename MapElem<MT>::raw4 (&r)[NS])
{
#pragma unroll
    for (int s = 0; s < NS; ++s)
        x[s] = widen4<MT>(r[s]);
}

__device__ __forceinline__ bool feature_live(float sq, float norm)
{
    return fabsf(sq) < __builtin_inff() && norm >= 1e-12f; // false for NaN
}

// the neighbour's two chains -> sim (header)
template <int NS>
__device__ __forceinline__ float similarity(const float4 (&a)[NS], const float4 (&b)[NS], bool valid, bool live_i, float norm_i)
{
    const float dot = wave_sum(lane_chain<NS>(a, b));
    const float sq = wave_sum(lane_chain<NS>(b, b));
    const float norm = __builtin_sqrtf(sq);
    const float s = dot / (norm_i * norm);
    return valid && live_i && feature_live(sq, norm) ? s : __builtin_nanf("");
}

template <int MT, bool VEC, int NS>
__global__ __launch_bounds__(256) void k_neighbor_similarity(int64_t N, int D, int k, const int32_t *__restrict__ idx,
                                                             const typename MapElem<MT>::raw *__restrict__ F, int64_t ldf,
                                                             float *__restrict__ sim, int32_t *__restrict__ live)
{
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); // wave-uniform
    if (g >= N)
        return;
    float4 a[NS], b0[NS], b1[NS];
    typename MapElem<MT>::raw4 r0[NS], r1[NS];
    load_row<MT, VEC, NS>(r0, F + g * ldf, lane, D);
    widen_row<MT, NS>(a, r0);
    const float sq_i = wave_sum(lane_chain<NS>(a, a));
    const float norm_i = __builtin_sqrtf(sq_i);
    const bool live_i = feature_live(sq_i, norm_i);
    const int32_t *row = idx + g * k;
    float *out = sim + g * k;
    for (int c = 0; c < k; c += 2) {
        const int j0 = (int)uniform((u32)row[c]);
        const int j1 = c + 1 < k ? (int)uniform((u32)row[c + 1]) : -1;
        const bool v0 = j0 >= 0 && j0 < N, v1 = j1 >= 0 && j1 < N;
        load_row<MT, VEC, NS>(r0, v0 ? F + (int64_t)j0 * ldf : nullptr, lane, D);
        load_row<MT, VEC, NS>(r1, v1 ? F + (int64_t)j1 * ldf : nullptr, lane, D);
        widen_row<MT, NS>(b0, r0);
        widen_row<MT, NS>(b1, r1);
        const float s0 = similarity<NS>(a, b0, v0, live_i, norm_i);
        const float s1 = similarity<NS>(a, b1, v1, live_i, norm_i);
        if (lane == 0) {
            out[c] = s0;
            if (c + 1 < k)
                out[c + 1] = s1;
        }
    }
    if (lane == 0)
        live[g] = live_i ? 1 : 0;
}

// lane = row i; the edges of its list (header)
__global__ __launch_bounds__(kUnionThreads) void k_edge_union(int64_t N, int k, const int32_t *__restrict__ idx,
                                                              const float *__restrict__ sim, const int32_t *__restrict__ live,
                                                              const float *__restrict__ dist, const int32_t *__restrict__ group,
                                                              float sim_min, float max_dist, int32_t *__restrict__ count,
                                                              int32_t *parent, int32_t *status)
{
    const int64_t i = (int64_t)blockIdx.x * kUnionThreads + threadIdx.x;
    if (i >= N)
        return;
    const int gi = group ? group[i] : 0;
    const bool live_i = live[i] != 0 && gi >= 0;
    count[i] = live_i ? 1 : 0;
    if (!live_i)
        return;
    const int cap = (int)min(N + 1, (int64_t)0x7FFFFFFF);
    int mine = (int)i; // an ancestor of i: where the next find starts
    for (int c = 0; c < k; ++c) {
        const int j = idx[i * k + c];
        if (j < 0 || j >= N || j == i)
            continue;
        if (!(sim[i * k + c] >= sim_min)) // (NaN fails: j is not feature-live)
            continue;
        if (dist && !(dist[i * k + c] <= max_dist))
            continue;
        if (group && group[j] != gi)
            continue;
        mine = uf_unite(parent, mine, j, cap, status);
    }
}

// the third dispatch level, particular to this kernel: CH 256-channel steps per row held in registers
template <int MT, bool VEC>
void launch_similarity(unsigned grid, hipStream_t s, int64_t N, int D, int k, const int32_t *idx, const void *Fv, int64_t ldf,
                       float *sim, int32_t *live)
{
    const auto F = field_ptr<MT>(Fv);
    if (D <= 256)
        hipLaunchKernelGGL((k_neighbor_similarity<MT, VEC, 1>), dim3(grid), dim3(256), 0, s, N, D, k, idx, F, ldf, sim, live);
    else if (D <= 512)
        hipLaunchKernelGGL((k_neighbor_similarity<MT, VEC, 2>), dim3(grid), dim3(256), 0, s, N, D, k, idx, F, ldf, sim, live);
    else if (D <= 1024)
        hipLaunchKernelGGL((k_neighbor_similarity<MT, VEC, 4>), dim3(grid), dim3(256), 0, s, N, D, k, idx, F, ldf, sim, live);
    else
        hipLaunchKernelGGL((k_neighbor_similarity<MT, VEC, 8>), dim3(grid), dim3(256), 0, s, N, D, k, idx, F, ldf, sim, live);
}

} // namespace

int launch_neighbor_similarity(int64_t N, int D, int k, const int32_t *idx, const void *F, int mt, int64_t ldf, float *sim,
                               int32_t *live, hipStream_t s)
{
    const unsigned grid = (unsigned)((N + 3) / 4); // (N < 2^31, checked by the caller)
    with_field_type(mt, field_rows_vec(F, ldf, mt),
                    [&](auto MT, auto VEC) { launch_similarity<MT, VEC>(grid, s, N, D, k, idx, F, ldf, sim, live); });
    return check_hip(hipGetLastError(), "neighbor_similarity launch");
}

int launch_edge_union(int64_t N, int k, const int32_t *idx, const float *sim, const int32_t *live, const float *dist,
                      const int32_t *group, float sim_min, float max_dist, int32_t *count, int32_t *parent, int32_t *status,
                      hipStream_t s)
{
    const unsigned grid = (unsigned)((N + kUnionThreads - 1) / kUnionThreads);
    if (!(max_dist < __builtin_inff()))
        dist = nullptr; // +inf: no cut
    hipLaunchKernelGGL(k_edge_union, dim3(grid), dim3(kUnionThreads), 0, s, N, k, idx, sim, live, dist, group, sim_min, max_dist, count,
                       parent, status);
    return check_hip(hipGetLastError(), "edge_union launch");
}

} // namespace gwbp
