// knn.hip -- k_knn_search: exact inner-product k-nearest-neighbour search of N query rows against M source rows (faiss's
// IndexFlatIP.search), scores and running top-k fused in one kernel; k_knn_vote: the majority label of each row's neighbours.
//
//   score(g, j) = <Q[g, :], S[j, :]>,   idx[g, 0..k-1] = the k sources of largest score, score desc, then index asc
//
// The reference does this with faiss on the CPU (affordance_transfer/demo_affordance_transfer.py:1377-1396, k = 5; :852-867,
// k = 20).  Here no score ever reaches global memory: a workgroup owns 128 queries, streams all of S through LDS in tiles of 128
// sources, finishes each 128 x 128 score tile over the full D on the fp32 matrix cores, drops it into LDS (over the operand
// staging, which is idle by then) and lets the thread that owns a query scan its row against the query's current k-th best.
//
// ARITHMETIC CONTRACT (the staging and the MFMA tile are knn_tile.h, shared with cluster.hip's k_kmeans_assign).  A score is ONE
// chain of fp32 fused multiply-adds over the D index, starting from +0, in an order that depends only on D:
// v_mfma_f32_16x16x4_f32 is bit for bit a k-ordered chain of fmaf (see encode.hip), and every output element
// of every tile consumes k = 32 c + 16 b + 4 q + i in the order (c, b, i, q) -- chunk, 16-block, MFMA step, slot.  Columns D ..
// 32 ceil(D / 32) - 1 are zero-filled in LDS for queries and sources alike (fmaf(0, 0, acc) == acc).  The chain does not depend on
// the row's position in Q or S, on N, M, k or the grid, so: permuting Q's rows permutes the result rows bit for bit; identical
// source rows get bit-equal scores; a zero query row scores exactly +0 against every finite source.  No reduced-precision operand.
//
// ORDER.  Candidates are compared as 64-bit keys (monotone map of the score's bits) << 32 | ~index: larger score first, equal
// scores (-0 counts as +0) by ascending index.  A NaN score (a NaN, or 0 x inf, in either row) maps to the lowest key: NaN scores
// order after every number, among themselves by ascending index, and are returned as NaN.
//
// Every loop has a trip count that is uniform over the workgroup (tiles, chunks, k, the 128 columns of a score row); the rare
// insert runs under a lane mask inside such a loop, never as a loop of its own.
#include "gwbp_dev.h"
#include "knn_tile.h"

namespace gwbp {

namespace {

constexpr int kKnnMaxK = 32;

template <int QT, bool VEC>
__global__ __launch_bounds__(kKnnThreads) void k_knn_search(int64_t N, int M, int D, int k,
                                                            const typename MapElem<QT>::raw *__restrict__ Q, int64_t ldq,
                                                            const float *__restrict__ S, int64_t lds_,
                                                            int32_t *__restrict__ idx, float *__restrict__ score)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    u64 *list = reinterpret_cast<u64 *>(smem + 2 * kKnnStage);    // [k][kKnnQ] keys of the running top-k, unordered

    const int tid = threadIdx.x;
    const int64_t q0 = (int64_t)blockIdx.x * kKnnQ;

    // selection role (threads 0..127): query q0 + tid, its k-th best key and that key's score
    u64 thr = 0;
    float thr_f = __uint_as_float(0x7FC00000u);
    int thr_at = 0;
    if (tid < kKnnQ)
        for (int j = 0; j < k; ++j)
            list[j * kKnnQ + tid] = 0; // below every candidate: key 0 with index 0xFFFFFFFF

    knn_score_tiles<QT, VEC>(N, M, D, Q, ldq, S, lds_, smem, [&](int tile, const float *sc) {
        if (tid < kKnnQ) {
            const u32 s0 = (u32)tile * kKnnS;
            const float *row = sc + tid * kKnnScoreLd;
            for (int c = 0; c < kKnnS; c += 4) { // uniform trip count; columns at or beyond M are masked
                const float4 v = *reinterpret_cast<const float4 *>(row + c);
                const float vs[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const u32 j = s0 + c + u;
                    // a score below the k-th best is out (almost every one after the first tiles); equal, NaN, or an open
                    // list (thr_f NaN) go on to the exact comparison of the keys
                    if (j < (u32)M && !(vs[u] < thr_f)) {
                        const u64 key = ((u64)score_key(vs[u]) << 32) | (u64)(0xFFFFFFFFu - j);
                        if (key > thr) {
                            list[thr_at * kKnnQ + tid] = key; // replaces the k-th best; find the new one
                            u64 lo = key;
                            int at = thr_at;
                            for (int t = 0; t < k; ++t) {
                                const u64 e = list[t * kKnnQ + tid];
                                if (e < lo) {
                                    lo = e;
                                    at = t;
                                }
                            }
                            thr = lo;
                            thr_at = at;
                            thr_f = key_score((u32)(lo >> 32));
                        }
                    }
                }
            }
        }
    });

    // the k keys of each query in descending order: k passes, each takes the largest key that is left
    if (tid < kKnnQ && q0 + tid < N) {
        const int64_t g = q0 + tid;
        for (int o = 0; o < k; ++o) {
            u64 hi = 0;
            int at = 0;
            for (int t = 0; t < k; ++t) {
                const u64 e = list[t * kKnnQ + tid];
                if (e > hi) {
                    hi = e;
                    at = t;
                }
            }
            list[at * kKnnQ + tid] = 0;
            idx[g * k + o] = (int32_t)(0xFFFFFFFFu - (u32)hi);
            score[g * k + o] = key_score((u32)(hi >> 32));
        }
    }
}

// One thread per query row: the most frequent label among labels[idx[g, 0..k-1]], the smallest of equally frequent ones
// (np.bincount(row).argmax()); labels outside [0, num_classes) and indices outside [0, M) are ignored, a row with none left gets
// -1.  counts (optional): the row's histogram, counts[g * ldc + c].
__global__ __launch_bounds__(256) void k_knn_vote(int64_t N, int M, int k, const int32_t *__restrict__ idx,
                                                  const int32_t *__restrict__ labels, int num_classes,
                                                  int32_t *__restrict__ label_out, int32_t *__restrict__ counts, int64_t ldc)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= N)
        return;
    int lab[kKnnMaxK];
#pragma unroll
    for (int j = 0; j < kKnnMaxK; ++j) {
        int l = -1;
        if (j < k) {
            const int i = idx[g * k + j];
            if (i >= 0 && i < M)
                l = labels[i];
            if (l < 0 || l >= num_classes)
                l = -1;
        }
        lab[j] = l;
    }
    int best = -1, best_n = 0;
#pragma unroll
    for (int j = 0; j < kKnnMaxK; ++j) {
        int n = 0;
#pragma unroll
        for (int i = 0; i < kKnnMaxK; ++i)
            n += (lab[i] == lab[j]) ? 1 : 0;
        if (lab[j] >= 0 && (n > best_n || (n == best_n && lab[j] < best))) {
            best = lab[j];
            best_n = n;
        }
    }
    label_out[g] = best;
    if (counts) {
        int32_t *row = counts + g * ldc;
        for (int c = 0; c < num_classes; ++c)
            row[c] = 0;
#pragma unroll
        for (int j = 0; j < kKnnMaxK; ++j)
            if (lab[j] >= 0)
                row[lab[j]] += 1;
    }
}

} // namespace

int launch_knn_search(int64_t N, int M, int D, int k, const void *Q, int mt, int64_t ldq, const float *S, int64_t lds_, int32_t *idx,
                      float *score, hipStream_t s)
{
    if (N == 0)
        return GWBP_OK;
    unsigned grid;
    if (int rc = grid_of("knn_search", N, &grid, kKnnQ))
        return rc;
    const bool vec = field_rows_vec(Q, ldq, mt) && field_rows_vec(S, lds_, GWBP_MAP_F32);
    const int lds_max = 2 * kKnnStage * (int)sizeof(float) + kKnnMaxK * kKnnQ * (int)sizeof(u64); // the largest request (k = 32)
    const size_t lds = 2 * kKnnStage * sizeof(float) + (size_t)k * kKnnQ * sizeof(u64);
    return with_field_type(mt, vec, [&](auto QT, auto VEC) {
        if (int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(k_knn_search<QT, VEC>), lds_max))
            return rc;
        hipLaunchKernelGGL((k_knn_search<QT, VEC>), dim3(grid), dim3(kKnnThreads), lds, s, N, M, D, k, field_ptr<QT>(Q), ldq, S, lds_, idx,
                           score);
        return check_hip(hipGetLastError(), "knn_search launch");
    });
}

int launch_knn_vote(int64_t N, int M, int k, const int32_t *idx, const int32_t *labels, int num_classes, int32_t *label_out,
                    int32_t *counts, int64_t ldc, hipStream_t s)
{
    if (N == 0)
        return GWBP_OK;
    unsigned grid;
    if (int rc = grid_of("knn_vote", N, &grid, 256))
        return rc;
    hipLaunchKernelGGL(k_knn_vote, dim3(grid), dim3(256), 0, s, N, M, k, idx, labels, num_classes, label_out, counts,
                       ldc);
    return check_hip(hipGetLastError(), "knn_vote launch");
}

} // namespace gwbp
