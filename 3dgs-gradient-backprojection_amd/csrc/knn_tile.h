// knn_tile.h -- the 128 x 128 inner-product score tile that k_knn_search (knn.hip) and k_kmeans_assign (cluster.hip) share: a
// workgroup owns 128 query rows, streams the M source rows through LDS in tiles of 128, finishes each score tile over the full D on
// the fp32 matrix cores, drops it into LDS (over the operand staging, which is idle by then) and hands it to the caller's selection.
//
// ARITHMETIC CONTRACT.  A score is ONE chain of fp32 fused multiply-adds over the D index, starting from +0, in an order that
// depends only on D: v_mfma_f32_16x16x4_f32 is bit for bit a k-ordered chain of fmaf (see encode.hip), and every output element
// of every tile consumes k = 32 c + 16 b + 4 q + i in the order (c, b, i, q) -- chunk, 16-block, MFMA step, slot.  Columns D ..
// 32 ceil(D / 32) - 1 are zero-filled in LDS for queries and sources alike (fmaf(0, 0, acc) == acc).  The chain does not depend on
// the row's position in Q or S, on N, M, the selection or the grid.  No reduced-precision operand.
//
// Every loop has a trip count that is uniform over the workgroup (tiles, chunks); rows and columns beyond N, M and D are masks.
#pragma once
#include "gwbp_dev.h"

namespace gwbp {

constexpr int kKnnThreads = 256;         // 4 waves, 2 (queries) x 2 (sources); each wave owns a 64 x 64 block of the score tile
constexpr int kKnnQ = 128;               // queries per workgroup
constexpr int kKnnS = 128;               // sources per tile
constexpr int kKnnKC = 32;               // D-chunk staged per step
constexpr int kKnnLd = kKnnKC + 4;       // LDS row stride of a staged chunk (floats): 16 rows x ds_read_b128 hit 64 distinct banks
constexpr int kKnnScoreLd = kKnnS + 4;   // LDS row stride of the score tile
constexpr int kKnnStage = (kKnnQ + kKnnS) * kKnnLd; // floats of one staging buffer (queries, then sources)
static_assert(2 * kKnnStage >= kKnnQ * kKnnScoreLd, "the score tile lies over the two staging buffers");

typedef float knn_f32x4 __attribute__((ext_vector_type(4)));

// Monotone map of a score's bits to an unsigned key: a larger score gives a larger key, -0 counts as +0, NaN gives the lowest key.
__device__ __forceinline__ u32 score_key(float s)
{
    if (s != s)
        return 0u;
    const u32 b = __float_as_uint(s + 0.0f); // -0 -> +0
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_score(u32 key)
{
    if (key == 0u)
        return __uint_as_float(0x7FC00000u);
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
}

// Runs the workgroup's 128 queries (rows blockIdx.x * 128 ... of Q) against every tile of S.  smem: 2 * kKnnStage floats, 16-B
// aligned.  select(tile, sc) is called by all 256 threads once per tile, between two barriers, with sc[q * kKnnScoreLd + s] = the
// score of query q of the workgroup against source tile * 128 + s (rows beyond N and sources beyond M hold scores of zero rows:
// the selection masks them).  QT: the element type of Q, the field operand (a half row is widened as it is loaded, so the staged
// values and every chain are those of the fp32 tile on the widened rows); S is fp32.  VEC: both operands take their vector loads.
template <int QT, bool VEC, class Select>
__device__ __forceinline__ void knn_score_tiles(int64_t N, int M, int D, const typename MapElem<QT>::raw *__restrict__ Q, int64_t ldq,
                                                const float *__restrict__ S, int64_t lds_, float *smem, Select select)
{
    float *stage = smem; // [2][kKnnQ + kKnnS][kKnnLd]; the score tile lies over it

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wq = wave >> 1, ws = wave & 1;
    const int m = lane & 15, qd = lane >> 4;
    const int64_t q0 = (int64_t)blockIdx.x * kKnnQ;

    // staging role: float4 column c4 of rows r0 + 32 i (i < 4) of the query block and of the source tile
    const int c4 = (tid & 7) * 4, r0 = tid >> 3;
    const typename MapElem<QT>::raw *qrow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t g = q0 + r0 + 32 * i;
        qrow[i] = g < N ? Q + g * ldq : nullptr;
    }

    const int n_chunk = (D + kKnnKC - 1) / kKnnKC;
    const int n_tile = (M + kKnnS - 1) / kKnnS;
    const int64_t n_it = (int64_t)n_tile * n_chunk;

    typename MapElem<QT>::raw4 pq[4]; // (the bits as loaded: widened where the staging writes them)
    float4 ps[4];
    auto prefetch = [&](int tile, int chunk) {
        const int c = chunk * kKnnKC + c4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            pq[i] = load4raw<QT, VEC>(qrow[i], c, D);
            const u32 j = (u32)tile * kKnnS + r0 + 32 * i; // (M < 2^31: no wrap)
            ps[i] = load4<VEC>(j < (u32)M ? S + (int64_t)j * lds_ : nullptr, c, D);
        }
    };
    prefetch(0, 0);

    knn_f32x4 acc[4][4]; // [source block a][query block b]: lane holds query 16 b + m, sources 16 a + 4 qd + r
    int tile = 0, chunk = 0;
    for (int64_t it = 0; it < n_it; ++it) {
        if (chunk == 0) {
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    acc[a][b] = knn_f32x4{0.f, 0.f, 0.f, 0.f};
        }
        float *buf = stage + (it & 1) * kKnnStage;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<float4 *>(buf + (r0 + 32 * i) * kKnnLd + c4) = widen4<QT>(pq[i]);
            *reinterpret_cast<float4 *>(buf + (kKnnQ + r0 + 32 * i) * kKnnLd + c4) = ps[i];
        }
        __syncthreads();
        int ntile = tile, nchunk = chunk + 1;
        if (nchunk == n_chunk) {
            nchunk = 0;
            ++ntile;
        }
        if (it + 1 < n_it)
            prefetch(ntile, nchunk); // in flight beside this chunk's MFMAs

        const float *bq = buf + (wq * 64 + m) * kKnnLd + 4 * qd;
        const float *bs = buf + (kKnnQ + ws * 64 + m) * kKnnLd + 4 * qd;
#pragma unroll
        for (int kb = 0; kb < kKnnKC / 16; ++kb) {
            float4 fa[4], fb[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                fa[a] = *reinterpret_cast<const float4 *>(bs + a * 16 * kKnnLd + kb * 16);
                fb[a] = *reinterpret_cast<const float4 *>(bq + a * 16 * kKnnLd + kb * 16);
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[a].x, fb[b].x, acc[a][b], 0, 0, 0);
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[a].y, fb[b].y, acc[a][b], 0, 0, 0);
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[a].z, fb[b].z, acc[a][b], 0, 0, 0);
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[a].w, fb[b].w, acc[a][b], 0, 0, 0);
        }

        if (chunk == n_chunk - 1) {
            // the tile's scores are complete: drop them into LDS as tile[query][source] and select
            __syncthreads(); // every wave is done reading the staging buffers
            float *sc = smem;
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    *reinterpret_cast<knn_f32x4 *>(sc + (wq * 64 + b * 16 + m) * kKnnScoreLd + ws * 64 + a * 16 + 4 * qd) = acc[a][b];
            __syncthreads();
            select(tile, sc);
            __syncthreads(); // the score tile is consumed before the next chunk is staged over it
        }
        tile = ntile;
        chunk = nchunk;
    }
}

} // namespace gwbp
