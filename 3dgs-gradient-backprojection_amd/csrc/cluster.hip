// cluster.hip -- the two [N, D] passes of a Lloyd step on a finished feature field:
//
//   k_kmeans_assign   label[g] = argmax_j  <X[g, :], C[j, :]> + b[j],  best[g] = that score          (j < K centroids)
//   k_cluster_sums    sums[k, c] = sum_{g: label[g] = k} w[g] X[g, c],  wsum[k] = sum w[g]           (float64, no atomics)
//
// ASSIGNMENT.  The inner product is k_knn_search's score, bit for bit: the staging and the 128 x 128 MFMA tile are knn_tile.h's,
// one chain of fp32 fused multiply-adds over the D index in an order that depends only on D.  b == nullptr: the score is the chain
// (cosine / inner-product metric).  Otherwise ONE fp32 addition of b[j] follows the finished chain; b[j] = -|c_j|^2 / 2 makes the
// argmax the Euclidean nearest centroid.  Ties go to the lowest index, -0 counts as +0 (best is returned as +0), a NaN score is
// never chosen: a row whose scores are all NaN gets label -1 and best NaN.  The running best is two registers per thread: thread t
// scans columns 64 (t / 128) ... + 63 of query t % 128 of every score tile, and the two halves of a query meet once, at the end,
// through one LDS slot each.  No key list.
//
// SUMS.  The caller has grouped the rows: order[N] lists them by label ascending (row index ascending inside a label: a stable
// sort), start[k] is the first position of label k, start[K] the end of label K - 1; labels outside [0, K) lie outside
// [start[0], start[K]) and take no part.  A cluster's member list is cut into runs of kRun members.  A wave owns one run and
// 256 columns (a lane: four consecutive ones), and adds the run's terms (double)w * (double)x -- exact: 24 x 24 bits -- to ONE
// float64 accumulator per column in ascending member order, eight gathered rows in flight.  k_cluster_reduce then adds a cluster's
// runs in ascending order in float64.  The result depends on (X, labels, w) alone: not on the launch, not on where the cluster lies
// in `order`, not on alignment (rows whose addresses and stride are 16-B aligned are read with 16-B loads, others element by
// element: same values, same chains).  Two runs give the same bits.
//
// Every loop has a trip count that is uniform over the wave (tiles, chunks, the 64 columns of a half score row, the members of a
// run, the runs of a cluster, the steps of a binary search on uniform values); bounds are lane masks inside them.  No spin loops.
#include "gwbp_dev.h"
#include "knn_tile.h"

namespace gwbp {

namespace {

// ---- assignment -----------------------------------------------------------------------------------------------------------------
// MT (both kernels): the element type of X, widened as it is loaded; centroids, bias, weights and every output are what they were
template <int MT, bool VEC>
__global__ __launch_bounds__(kKnnThreads) void k_kmeans_assign(int64_t N, int K, int D,
                                                               const typename MapElem<MT>::raw *__restrict__ X, int64_t ldx,
                                                               const float *__restrict__ C, int64_t ldc,
                                                               const float *__restrict__ bias, int32_t *__restrict__ label,
                                                               float *__restrict__ best)
{
    extern __shared__ __attribute__((aligned(16))) float smem[]; // 2 * kKnnStage floats: the staging, the score tile over it

    const int tid = threadIdx.x;
    const int q = tid & (kKnnQ - 1), half = tid >> 7; // (half is uniform over a wave)
    const int64_t q0 = (int64_t)blockIdx.x * kKnnQ;

    float bv = 0.f; // the running best of this thread's half of query q0 + q; bj < 0: none yet
    int bj = -1;

    knn_score_tiles<MT, VEC>(N, K, D, X, ldx, C, ldc, smem, [&](int tile, const float *sc) {
        const int s0 = tile * kKnnS + half * (kKnnS / 2);
        const float *row = sc + q * kKnnScoreLd + half * (kKnnS / 2);
        for (int c = 0; c < kKnnS / 2; c += 4) { // uniform trip count; columns at or beyond K are masked
            const float4 v = *reinterpret_cast<const float4 *>(row + c);
            const float vs[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = s0 + c + u;
                const bool in = j < K;
                float s = vs[u];
                if (bias)
                    s += in ? bias[j] : 0.f;
                // ascending j: a later equal score (-0 == +0) does not replace; NaN compares false and is never taken
                if (in && (s > bv || (bj < 0 && s == s))) {
                    bv = s;
                    bj = j;
                }
            }
        }
    });

    // the two halves of a query: the upper half parks its best in LDS (the tile loop ended with a barrier), the lower one decides
    float *pv = smem;
    int *pj = reinterpret_cast<int *>(smem + kKnnQ);
    if (half == 1) {
        pv[q] = bv;
        pj[q] = bj;
    }
    __syncthreads();
    if (half == 0 && q0 + q < N) {
        const float ov = pv[q];
        const int oj = pj[q];
        if (oj >= 0 && (bj < 0 || ov > bv || (ov == bv && oj < bj))) {
            bv = ov;
            bj = oj;
        }
        label[q0 + q] = bj;
        best[q0 + q] = bj < 0 ? __uint_as_float(0x7FC00000u) : bv + 0.0f; // (-0 -> +0, as k_knn_search returns it)
    }
}

// ---- sums -----------------------------------------------------------------------------------------------------------------------
constexpr int kRun = GWBP_CLUSTER_RUN;   // members per run: part of the arithmetic contract
constexpr int kSumWaves = 4;             // runs per workgroup (one per wave)
constexpr int kSumCols = 256;            // columns per wave: 64 lanes x 4
constexpr int kSumFlight = 8;            // gathered rows in flight per wave
constexpr int kScanThreads = 256;

// Upper bound of the number of non-empty runs: every cluster with n_k members has ceil(n_k / kRun) <= n_k / kRun + 1 of them, and
// no more than n_k.
int64_t run_slots(int64_t N, int K)
{
    const int64_t a = (N + kRun - 1) / kRun + K;
    const int64_t s = a < N ? a : N;
    return s > 0 ? s : 1;
}

struct SumWs {
    int64_t *run_start; // [K + 1]: the first run slot of every cluster
    double *wpartial;   // [slots]
    double *partial;    // [slots][D]
    size_t bytes;
};
SumWs sum_ws(void *ws, int64_t N, int D, int K)
{
    const int64_t slots = run_slots(N, K);
    const size_t a = ((size_t)(K + 1) * sizeof(int64_t) + 255) & ~(size_t)255;
    const size_t b = ((size_t)slots * sizeof(double) + 255) & ~(size_t)255;
    char *p = static_cast<char *>(ws);
    SumWs w;
    w.run_start = reinterpret_cast<int64_t *>(p);
    w.wpartial = reinterpret_cast<double *>(p + a);
    w.partial = reinterpret_cast<double *>(p + a + b);
    w.bytes = a + b + (size_t)slots * D * sizeof(double);
    return w;
}

// Every start[] value is clamped into [0, N] where it is read: whatever the caller passed, a run reads positions inside [0, N).
__device__ __forceinline__ int64_t clamp_pos(int64_t p, int64_t N) { return p < 0 ? 0 : (p > N ? N : p); }
__device__ __forceinline__ int64_t members_of(const int64_t *__restrict__ start, int k, int64_t N)
{
    const int64_t lo = clamp_pos(start[k], N), hi = clamp_pos(start[k + 1], N);
    return hi > lo ? hi - lo : 0;
}

// run_start[k] = sum_{j < k} ceil(n_j / kRun), k <= K.  One workgroup: thread t owns clusters t * per .. t * per + per - 1.
__global__ __launch_bounds__(kScanThreads) void k_cluster_runs(int64_t N, int K, const int64_t *__restrict__ start,
                                                               int64_t *__restrict__ run_start)
{
    __shared__ int64_t tot[kScanThreads];
    const int t = threadIdx.x;
    const int per = (K + kScanThreads - 1) / kScanThreads;
    const int k0 = t * per;
    int64_t mine = 0;
    for (int i = 0; i < per; ++i) { // uniform trip count
        const int k = k0 + i;
        if (k < K)
            mine += (members_of(start, k, N) + kRun - 1) / kRun;
    }
    tot[t] = mine;
    __syncthreads();
    int64_t base = 0;
    for (int i = 0; i < kScanThreads; ++i) // uniform trip count
        base += i < t ? tot[i] : 0;
    for (int i = 0; i < per; ++i) {
        const int k = k0 + i;
        if (k < K) {
            run_start[k] = base;
            base += (members_of(start, k, N) + kRun - 1) / kRun;
        }
    }
    if (t == kScanThreads - 1)
        run_start[K] = base; // (the last thread's clusters are the last ones: its base is the total)
}

template <int MT, bool VEC>
__global__ __launch_bounds__(64 * kSumWaves) void k_cluster_sums(int64_t N, int D, int K, int64_t slots,
                                                                  const typename MapElem<MT>::raw *__restrict__ X, int64_t ldx,
                                                                  const float *__restrict__ w, const int64_t *__restrict__ order,
                                                                  const int64_t *__restrict__ start,
                                                                  const int64_t *__restrict__ run_start,
                                                                  double *__restrict__ partial, double *__restrict__ wpartial)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t slot = uniform64((u64)((int64_t)blockIdx.x * kSumWaves + wave));
    if (slot >= slots || slot >= run_start[K])
        return; // (no barrier below: a wave may leave)

    // the cluster of this run: the last k with run_start[k] <= slot (empty clusters repeat their successor's value)
    int lo = 0, hi = K; // invariant: run_start[lo] <= slot < run_start[hi]
    while (hi - lo > 1) { // values uniform over the wave
        const int mid = lo + ((hi - lo) >> 1);
        if (run_start[mid] <= slot)
            lo = mid;
        else
            hi = mid;
    }
    const int k = lo;
    const int64_t s_lo = clamp_pos(start[k], N), s_hi = clamp_pos(start[k + 1], N);
    const int64_t p0 = s_lo + (slot - run_start[k]) * kRun;
    const int64_t p1 = p0 + kRun < s_hi ? p0 + kRun : s_hi;

    const int c = (int)blockIdx.y * kSumCols + 4 * lane;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, aw = 0.0;
    for (int64_t p = p0; p < p1; p += kSumFlight) { // uniform trip count; positions at or beyond p1 are masked
        typename MapElem<MT>::raw4 v[kSumFlight]; // (the bits as loaded: eight rows in flight, widened where they are added)
        float wg[kSumFlight];
#pragma unroll
        for (int i = 0; i < kSumFlight; ++i) {
            const int64_t g = p + i < p1 ? order[p + i] : -1;
            const bool on = g >= 0 && g < N;
            v[i] = load4raw<MT, VEC>(on ? X + g * ldx : nullptr, c, D);
            wg[i] = on ? (w ? w[g] : 1.0f) : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < kSumFlight; ++i) { // ascending member order; a masked term adds +0
            const double wd = (double)wg[i];
            const float4 x = widen4<MT>(v[i]);
            a0 += wd * (double)x.x;
            a1 += wd * (double)x.y;
            a2 += wd * (double)x.z;
            a3 += wd * (double)x.w;
            aw += wd;
        }
    }
    double *out = partial + slot * D;
    if (c < D)
        out[c] = a0;
    if (c + 1 < D)
        out[c + 1] = a1;
    if (c + 2 < D)
        out[c + 2] = a2;
    if (c + 3 < D)
        out[c + 3] = a3;
    if (blockIdx.y == 0 && lane == 0)
        wpartial[slot] = aw;
}

// sums[k, :] and wsum[k]: the cluster's runs added in ascending order.  One workgroup per cluster.
__global__ __launch_bounds__(256) void k_cluster_reduce(int D, int64_t slots, const int64_t *__restrict__ run_start,
                                                        const double *__restrict__ partial, const double *__restrict__ wpartial,
                                                        double *__restrict__ sums, double *__restrict__ wsum)
{
    const int k = (int)blockIdx.x;
    const int64_t r0 = run_start[k], r1 = run_start[k + 1] < slots ? run_start[k + 1] : slots; // (slots: what was written)
    for (int c0 = 0; c0 < D; c0 += 256) { // uniform trip counts
        const int c = c0 + (int)threadIdx.x;
        double s = 0.0;
        for (int64_t r = r0; r < r1; ++r)
            s += c < D ? partial[r * D + c] : 0.0;
        if (c < D)
            sums[(int64_t)k * D + c] = s;
    }
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int64_t r = r0; r < r1; ++r)
            s += wpartial[r];
        wsum[k] = s;
    }
}

} // namespace

int launch_kmeans_assign(int64_t N, int K, int D, const void *X, int mt, int64_t ldx, const float *C, int64_t ldc, const float *bias,
                         int32_t *label, float *best, hipStream_t s)
{
    if (N == 0)
        return GWBP_OK;
    unsigned grid;
    if (int rc = grid_of("kmeans_assign", N, &grid, kKnnQ))
        return rc;
    const bool vec = field_rows_vec(X, ldx, mt) && field_rows_vec(C, ldc, GWBP_MAP_F32);
    const int lds = 2 * kKnnStage * (int)sizeof(float);
    return with_field_type(mt, vec, [&](auto MT, auto VEC) {
        if (int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(k_kmeans_assign<MT, VEC>), lds))
            return rc;
        hipLaunchKernelGGL((k_kmeans_assign<MT, VEC>), dim3(grid), dim3(kKnnThreads), lds, s, N, K, D, field_ptr<MT>(X), ldx, C, ldc,
                           bias, label, best);
        return check_hip(hipGetLastError(), "kmeans_assign launch");
    });
}

size_t cluster_workspace_bytes(int64_t N, int D, int K) { return sum_ws(nullptr, N, D, K).bytes; }

int launch_cluster_sums(int64_t N, int D, int K, const void *X, int mt, int64_t ldx, const float *w, const int64_t *order,
                        const int64_t *start, double *sums, double *wsum, void *ws, hipStream_t s)
{
    const SumWs W = sum_ws(ws, N, D, K);
    const int64_t slots = run_slots(N, K);
    unsigned grid;
    if (int rc = grid_of("cluster_sums", slots, &grid, kSumWaves))
        return rc;
    const int col_blocks = (D + kSumCols - 1) / kSumCols;
    if (col_blocks > 65535)
        return set_error(GWBP_EINVAL, "cluster_sums: D = %d needs more than 65535 column blocks", D);
    hipLaunchKernelGGL(k_cluster_runs, dim3(1), dim3(kScanThreads), 0, s, N, K, start, W.run_start);
    if (N > 0) {
        const dim3 g(grid, (unsigned)col_blocks);
        with_field_type(mt, field_rows_vec(X, ldx, mt), [&](auto MT, auto VEC) {
            hipLaunchKernelGGL((k_cluster_sums<MT, VEC>), g, dim3(64 * kSumWaves), 0, s, N, D, K, slots, field_ptr<MT>(X), ldx, w, order,
                               start, W.run_start, W.partial, W.wpartial);
        });
    }
    hipLaunchKernelGGL(k_cluster_reduce, dim3((unsigned)K), dim3(256), 0, s, D, slots, W.run_start, W.partial, W.wpartial, sums,
                       wsum);
    return check_hip(hipGetLastError(), "cluster_sums launch");
}

} // namespace gwbp
