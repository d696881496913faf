// sample.hip -- what a finished field says at an arbitrary 3-D point: the Gaussians that weigh on the point, by their own shape
// (scale, rotation, opacity), the field blended over them, and a weighted vote of their labels.  On the grid of spatial.hip with the
// ring walk of ring_walk.h.  (The reference has nothing of the kind; its users sample a field at the Gaussians' centres only.)
//
// THE CONTRACT (include/gwbp.h, DESIGN 4.0d and tests/sample_ref.py say the same).
//   LIVE(i): finite mean; finite quaternion with 0 < n2 < inf, n2 = fmaf(q3, q3, fmaf(q2, q2, fmaf(q1, q1, q0 * q0))); finite scales
//     > 0; finite opacity > 0; live[i] != 0 (no mask: every Gaussian).
//   PACK(i), fp32, every operation rounded once:  inv = 1 / sqrtf(n2);  (w, x, y, z) = (q0 inv, q1 inv, q2 inv, q3 inv);
//     x2 = x x, y2 = y y, z2 = z z, xy = x y, xz = x z, yz = y z, wx = w x, wy = w y, wz = w z;
//     R = [ 1 - 2 (y2 + z2)   2 (xy - wz)       2 (xz + wy)     ]
//         [ 2 (xy + wz)       1 - 2 (x2 + z2)   2 (yz - wx)     ]      (gsplat's quat_to_rotmat)
//         [ 2 (xz - wy)       2 (yz + wx)       1 - 2 (x2 + y2) ]
//     M[a][b] = R[b][a] / s[a];  o = opacity.  A dead Gaussian has M = 0, o = 0.
//     record (GWBP_SAMPLE_PACK = 12 floats, three float4): (M00 M01 M02 o) (M10 M11 M12 0) (M20 M21 M22 0), at the Gaussian's SORTED
//     position, so that a walk position indexes it and a cell's records sit together.
//   WEIGHT of Gaussian i at x:  d = x - mu (fp32, per component);  u_a = fmaf(M[a][2], d_z, fmaf(M[a][1], d_y, M[a][0] d_x));
//     m2 = fmaf(u_2, u_2, fmaf(u_1, u_1, u_0 u_0));  sigma = 0.5f m2;  w = o exp_neg(-sigma).  KEPT when sigma <= 80 and w >=
//     alpha_min, else 0.  (A dead Gaussian has w = 0 < alpha_min; a NaN sigma fails sigma <= 80.)
//   CANDIDATES of a query: the Gaussians with a finite mean and d2 <= r2 (d2: k_spatial_knn's expression).
//   RESULT: the k candidates of largest kept weight by (w descending, index ascending); idx tail -1, w tail 0; n_contrib = the
//     number of candidates with a kept weight.  A non-finite query gets the empty result.
// The walk's visiting order depends on the grid; the result does not: the list is the top k of a SET under a total order, the count is
// the size of a set, and nothing is summed across candidates.
//
// k_gaussian_pack: one lane per sorted position.
// k_point_gaussians: one lane per query, queries in the order of their cell keys (k_radius_count's shape).  The visitor loads the
//   record (three 16-B loads), computes w and offers it to the lane's sorted list in LDS, LaneTopK<HeaviestFirst> (lane_topk.h:
//   k_spatial_knn's list under the other order, k * threads * 8 bytes <= 32 KiB).  Lists are lane-private: no atomics, no waits.
// k_neighbor_blend: one wave per query, four per workgroup, lanes over channels four at a time (k_neighbor_mean's shape).  Lane j < k
//   reads entry j of the row's list once; the wave takes every entry from that lane by readlane (the loop index is wave-uniform).
//   W = the chain acc = w_j + acc from +0 over the entries that are not skipped, in list order; out[c] = (acc = fmaf(w_j, F[idx_j, c],
//   acc) from +0, same order) / W.  An entry with idx outside [0, m) or w == 0 is SKIPPED and its row is not read.  Rows are requested
//   two ahead (k_neighbor_similarity's pairs).  Every branch on an entry is wave-uniform.
// k_weighted_vote: one lane per query; the list's labels (-1 for an entry that takes no part) and weights staged in the lane's LDS
//   columns, then for each first occurrence of a class the chain of its weights in list order: O(k^2), no K-sized array.
#include "gwbp_dev.h"
#include "lane_topk.h"
#include "ring_walk.h"
#include "spatial_grid.h"

namespace gwbp {

namespace {

constexpr int kSampleThreads = 128; // lanes (queries) per workgroup of the walk and the vote; LDS = k * 128 * 8 B <= 32 KiB
constexpr int kPack4 = GWBP_SAMPLE_PACK / 4;
static_assert(GWBP_SAMPLE_PACK == 12, "the record is three float4");

__device__ __forceinline__ bool finite1(float x) { return fabsf(x) < __builtin_inff(); } // false for NaN

__global__ __launch_bounds__(256) void k_gaussian_pack(int64_t N, const float *__restrict__ means, int64_t ldm,
                                                       const float *__restrict__ quats, int64_t ldq, const float *__restrict__ scales,
                                                       int64_t lds_, const float *__restrict__ opac, const uint8_t *__restrict__ live,
                                                       const int64_t *__restrict__ perm, float4 *__restrict__ pack)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= N)
        return;
    const int64_t i = perm[p];
    const float q0 = quats[i * ldq], q1 = quats[i * ldq + 1], q2 = quats[i * ldq + 2], q3 = quats[i * ldq + 3];
    const float s0 = scales[i * lds_], s1 = scales[i * lds_ + 1], s2 = scales[i * lds_ + 2];
    const float o = opac[i];
    const float n2 = __builtin_fmaf(q3, q3, __builtin_fmaf(q2, q2, __builtin_fmaf(q1, q1, q0 * q0)));
    const bool ok = finite3(means[i * ldm], means[i * ldm + 1], means[i * ldm + 2]) && finite1(q0) && finite3(q1, q2, q3) &&
                    n2 > 0.0f && finite1(n2) && finite3(s0, s1, s2) && s0 > 0.0f && s1 > 0.0f && s2 > 0.0f && finite1(o) && o > 0.0f &&
                    (!live || live[i] != 0);
    float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0, r2 = r0;
    if (ok) {
        const float inv = 1.0f / __builtin_sqrtf(n2);
        const float w = q0 * inv, x = q1 * inv, y = q2 * inv, z = q3 * inv;
        const float x2 = x * x, y2 = y * y, z2 = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
        const float R00 = 1.0f - 2.0f * (y2 + z2), R01 = 2.0f * (xy - wz), R02 = 2.0f * (xz + wy);
        const float R10 = 2.0f * (xy + wz), R11 = 1.0f - 2.0f * (x2 + z2), R12 = 2.0f * (yz - wx);
        const float R20 = 2.0f * (xz - wy), R21 = 2.0f * (yz + wx), R22 = 1.0f - 2.0f * (x2 + y2);
        r0 = make_float4(R00 / s0, R10 / s0, R20 / s0, o); // M[a][b] = R[b][a] / s[a]
        r1 = make_float4(R01 / s1, R11 / s1, R21 / s1, 0.0f);
        r2 = make_float4(R02 / s2, R12 / s2, R22 / s2, 0.0f);
    }
    pack[p * kPack4] = r0;
    pack[p * kPack4 + 1] = r1;
    pack[p * kPack4 + 2] = r2;
}

__global__ __launch_bounds__(kSampleThreads) void k_point_gaussians(const float4 *__restrict__ S, const int32_t *__restrict__ cell_start,
                                                                    SpatialGrid G, const float4 *__restrict__ pack, float r2,
                                                                    float alpha_min, int64_t Q, const float *__restrict__ queries,
                                                                    int64_t ldq, const int64_t *__restrict__ order, int k,
                                                                    int32_t *__restrict__ idx, float *__restrict__ wout,
                                                                    int32_t *__restrict__ n_contrib, int32_t *__restrict__ visited)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int T = kSampleThreads;
    LaneTopK<HeaviestFirst, T> best(smem, k, threadIdx.x); // kept weights, descending

    const int64_t slot = (int64_t)blockIdx.x * T + threadIdx.x;
    if (slot >= Q)
        return; // (no barrier anywhere below)
    const int64_t g = order[slot];
    const float qx = queries[g * ldq], qy = queries[g * ldq + 1], qz = queries[g * ldq + 2];
    best.init();
    int nc = 0, seen = 0;
    if (finite3(qx, qy, qz))
        seen = radius_walk_at(S, cell_start, G, qx, qy, qz, r2, [&](float, const float4 &v, int p) {
            const float4 m0 = pack[(int64_t)p * kPack4], m1 = pack[(int64_t)p * kPack4 + 1], m2 = pack[(int64_t)p * kPack4 + 2];
            const float dx = qx - v.x, dy = qy - v.y, dz = qz - v.z;
            const float u0 = __builtin_fmaf(m0.z, dz, __builtin_fmaf(m0.y, dy, m0.x * dx));
            const float u1 = __builtin_fmaf(m1.z, dz, __builtin_fmaf(m1.y, dy, m1.x * dx));
            const float u2 = __builtin_fmaf(m2.z, dz, __builtin_fmaf(m2.y, dy, m2.x * dx));
            const float sigma = 0.5f * __builtin_fmaf(u2, u2, __builtin_fmaf(u1, u1, u0 * u0));
            const float w = m0.w * exp_neg(-sigma);
            if (!(sigma <= 80.0f && w >= alpha_min))
                return;
            ++nc;
            best.offer(w, __float_as_int(v.w));
        });
    for (int j = 0; j < k; ++j) {
        idx[g * k + j] = best.index(j);
        wout[g * k + j] = best.key(j); // (0 in an empty slot)
    }
    n_contrib[g] = nc;
    if (visited)
        visited[g] = seen;
}

__device__ __forceinline__ void fma4(float4 &acc, float w, const float4 &v)
{
    acc.x = __builtin_fmaf(w, v.x, acc.x);
    acc.y = __builtin_fmaf(w, v.y, acc.y);
    acc.z = __builtin_fmaf(w, v.z, acc.z);
    acc.w = __builtin_fmaf(w, v.w, acc.w);
}

// MT: the element type of F (a half row is widened as it is loaded; weights and chains are fp32); OT: that of out (a half out is the
// fp32 quotient rounded once, narrow<OT>)
template <int MT, int OT, bool VEC>
__global__ __launch_bounds__(256) void k_neighbor_blend(int64_t Q, int64_t M, int D, int k, const int32_t *__restrict__ idx,
                                                        const float *__restrict__ wts,
                                                        const typename MapElem<MT>::raw *__restrict__ F, int64_t ldf,
                                                        typename MapElem<OT>::raw *__restrict__ out, int64_t ldo,
                                                        float *__restrict__ wsum)
{
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); // wave-uniform
    if (g >= Q)
        return;
    // entry `lane` of the row's list, read once; an entry that is skipped becomes (-1, 0)
    int my_id = -1;
    float my_w = 0.0f;
    if (lane < k) {
        my_id = idx[g * k + lane];
        my_w = wts[g * k + lane];
        if (my_id < 0 || my_id >= M || my_w == 0.0f) {
            my_id = -1;
            my_w = 0.0f;
        }
    }
    float W = 0.0f;
    bool any = false;
    for (int j = 0; j < k; ++j) {
        const int id = __builtin_amdgcn_readlane(my_id, j);
        if (id < 0)
            continue;
        W = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_w), j)) + W;
        any = true;
    }
    if (lane == 0)
        wsum[g] = W;
    typename MapElem<OT>::raw *o = out + g * ldo;
    for (int c0 = 0; c0 < D; c0 += 256) {
        const int c = c0 + 4 * lane;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j < k; j += 2) {
            const int j0 = __builtin_amdgcn_readlane(my_id, j);
            const int j1 = j + 1 < k ? __builtin_amdgcn_readlane(my_id, j + 1) : -1;
            const float w0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_w), j));
            const float w1 = j + 1 < k ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_w), j + 1)) : 0.0f;
            // both rows requested before the first use (nullptr: no load)
            const auto r0 = load4raw<MT, VEC>(j0 >= 0 ? F + (int64_t)j0 * ldf : nullptr, c, D);
            const auto r1 = load4raw<MT, VEC>(j1 >= 0 ? F + (int64_t)j1 * ldf : nullptr, c, D);
            if (j0 >= 0)
                fma4(acc, w0, widen4<MT>(r0));
            if (j1 >= 0)
                fma4(acc, w1, widen4<MT>(r1));
        }
        if (any)
            acc = make_float4(acc.x / W, acc.y / W, acc.z / W, acc.w / W);
        store4t<OT, VEC>(o, c, D, acc);
    }
}

__global__ __launch_bounds__(kSampleThreads) void k_weighted_vote(int64_t Q, int64_t M, int k, const int32_t *__restrict__ idx,
                                                                  const float *__restrict__ wts, const int32_t *__restrict__ labels,
                                                                  int K, int32_t *__restrict__ out_label, float *__restrict__ out_share)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int T = kSampleThreads;
    const LaneColumns<T> col(smem, k, threadIdx.x);
    float *lw = col.f; // [k][T] the entries' weights
    int *lab = col.i;  // [k][T] their classes, -1 for an entry that takes no part
    const int64_t g = (int64_t)blockIdx.x * T + threadIdx.x;
    if (g >= Q)
        return; // (no barrier anywhere below)
    float total = 0.0f;
    for (int j = 0; j < k; ++j) {
        const int id = idx[g * k + j];
        const float w = wts[g * k + j];
        int c = -1;
        if (id >= 0 && id < M && w != 0.0f) {
            c = labels[id];
            if (c < 0 || c >= K)
                c = -1;
        }
        if (c >= 0)
            total = w + total;
        lw[j * T] = w;
        lab[j * T] = c;
    }
    int best = -1;
    float best_s = 0.0f;
    for (int j = 0; j < k; ++j) {
        const int c = lab[j * T];
        if (c < 0)
            continue;
        bool first = true;
        for (int e = 0; e < j; ++e)
            first = first && lab[e * T] != c;
        if (!first)
            continue;
        float s = 0.0f;
        for (int e = j; e < k; ++e)
            if (lab[e * T] == c)
                s = lw[e * T] + s;
        if (best < 0 || s > best_s || (s == best_s && c < best)) {
            best = c;
            best_s = s;
        }
    }
    out_label[g] = best;
    out_share[g] = best >= 0 ? best_s / total : 0.0f;
}

} // namespace

int launch_gaussian_pack(int64_t N, const float *means, int64_t ldm, const float *quats, int64_t ldq, const float *scales, int64_t lds_,
                         const float *opac, const uint8_t *live, const int64_t *perm, float *pack, hipStream_t s)
{
    unsigned grid;
    if (int rc = grid_of("gaussian_pack", N, &grid, 256))
        return rc;
    hipLaunchKernelGGL(k_gaussian_pack, dim3(grid), dim3(256), 0, s, N, means, ldm, quats, ldq, scales, lds_, opac, live, perm,
                       reinterpret_cast<float4 *>(pack));
    return check_hip(hipGetLastError(), "gaussian_pack launch");
}

int launch_point_gaussians(const float *sorted, const int32_t *cell_start, const float *lo, float h, const int32_t *dims,
                           const float *pack, float r2, float alpha_min, int64_t Q, const float *queries, int64_t ldq,
                           const int64_t *order, int k, int32_t *idx, float *w, int32_t *n_contrib, int32_t *visited, hipStream_t s)
{
    if (Q == 0)
        return GWBP_OK;
    unsigned grid;
    if (int rc = grid_of("point_gaussians", Q, &grid, kSampleThreads))
        return rc;
    const size_t lds = lane_columns_bytes(k, kSampleThreads); // <= 32 KiB: below the default limit
    hipLaunchKernelGGL(k_point_gaussians, dim3(grid), dim3(kSampleThreads), lds, s, reinterpret_cast<const float4 *>(sorted), cell_start,
                       make_grid(lo, h, dims), reinterpret_cast<const float4 *>(pack), r2, alpha_min, Q, queries, ldq, order, k, idx, w,
                       n_contrib, visited);
    return check_hip(hipGetLastError(), "point_gaussians launch");
}

int launch_neighbor_blend(int64_t Q, int64_t M, int D, int k, const int32_t *idx, const float *w, const void *F, int mt, int64_t ldf,
                          void *out, int ot, int64_t ldo, float *wsum, hipStream_t s)
{
    if (Q == 0)
        return GWBP_OK;
    unsigned grid;
    if (int rc = grid_of("neighbor_blend", Q, &grid, 4))
        return rc;
    const bool vec = field_rows_vec(F, ldf, mt) && field_rows_vec(out, ldo, ot);
    with_field_type(mt, vec, [&](auto MT, auto VEC) {
        with_map_type(ot, [&](auto OT) {
            hipLaunchKernelGGL((k_neighbor_blend<MT, OT, VEC>), dim3(grid), dim3(256), 0, s, Q, M, D, k, idx, w, field_ptr<MT>(F), ldf,
                               out_ptr<OT>(out), ldo, wsum);
        });
    });
    return check_hip(hipGetLastError(), "neighbor_blend launch");
}

int launch_weighted_vote(int64_t Q, int64_t M, int k, const int32_t *idx, const float *w, const int32_t *labels, int K,
                         int32_t *out_label, float *out_share, hipStream_t s)
{
    if (Q == 0)
        return GWBP_OK;
    unsigned grid;
    if (int rc = grid_of("weighted_vote", Q, &grid, kSampleThreads))
        return rc;
    const size_t lds = lane_columns_bytes(k, kSampleThreads);
    hipLaunchKernelGGL(k_weighted_vote, dim3(grid), dim3(kSampleThreads), lds, s, Q, M, k, idx, w, labels, K, out_label, out_share);
    return check_hip(hipGetLastError(), "weighted_vote launch");
}

} // namespace gwbp
