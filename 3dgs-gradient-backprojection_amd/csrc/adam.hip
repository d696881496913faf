// adam.hip -- the optimiser step of training: Adam on one [n, w] float32 table in place, with an optional row mask.
// adam_math.h carries every expression that is not a memory access.
//
//   k_adam_step<MASKED>   p, m, v [n, w] updated from g [n, w]; MASKED: only the rows i with visible[i] != 0 (uint8 [n]).
//
// Memory shape.  The table is walked flat, in 16-B chunks (the four tables are 16-B aligned, so chunk q is elements 4 q .. 4 q + 3 of
// each): a workgroup takes a tile of kAdamBatch x 256 consecutive chunks per turn, consecutive lanes on consecutive chunks, and a thread
// issues its kAdamBatch global_load_dwordx4 of p, g, m and v before it waits for the first (one chunk per turn would leave every wave
// with four loads in flight; see the kShBatch note in sh.hip).  The grid is the device's (CUs x kAdamWgsPerCu workgroups at most) and
// strides over the tiles.  The byte floor is 28 B per float: four loads, three stores.
//
// The mask.  A chunk's elements lie in rows (4 q + j) / w; w % 4 == 0 keeps a chunk inside one row, any other w (1, 3, 45) lets it
// straddle up to four.  A chunk whose rows are ALL invisible issues no load and no store of p, g, m, v: its mask bytes are its only
// traffic.  A chunk with at least one visible row is loaded whole, the update is computed for all four elements, each element then
// takes the new value where its row is visible and the LOADED bits where it is not (a select, bit-preserving), and the chunk is stored
// whole with three 16-B stores.  A chunk has exactly one owner, so writing an invisible element's own bits back races with nobody,
// and an invisible row keeps the bits of all three tables either way.  The up to three elements behind the last whole chunk
// (n w % 4) go through scalar loads and stores in workgroup 0.
//
// No atomics, no LDS, nothing between workgroups: the result is a function of the inputs alone, the same bits every run.  Every index
// is below n w (q < n4 = n w / 4, so 4 q + 3 < n w) and every row below n; loop bounds are kernel arguments.
#include "gwbp_dev.h"
#include "adam_math.h"

namespace gwbp {

namespace {

constexpr int kAdamBlock = 256;
constexpr int kAdamBatch = 4;     // 16-B chunks of each table a thread keeps in flight (16 loads, 64 VGPRs)
constexpr int kAdamWgsPerCu = 8;  // the grid's cap per CU: at least the 4 to 5 workgroups a CU holds at once (94 to 108 VGPRs)

// row of element e; `narrow`: n w < 2^32, a 32-bit division (the same for every thread)
__device__ __forceinline__ u64 adam_row(u64 e, u32 w, bool narrow) { return narrow ? (u64)((u32)e / w) : e / w; }

// bit j: element 4 q + j lies in a visible row
__device__ __forceinline__ unsigned adam_chunk_mask(const uint8_t *__restrict__ visible, u64 q, u32 w, bool narrow)
{
    const u64 e0 = 4 * q;
    u64 r = adam_row(e0, w, narrow);
    u32 c = (u32)(e0 - r * w);
    unsigned on = visible[r] != 0, bits = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        bits |= on << j;
        if (j < 3 && ++c == w) {
            c = 0;
            on = visible[++r] != 0; // (element 4 q + j + 1 <= 4 q + 3 < n w: row r < n)
        }
    }
    return bits;
}

__device__ __forceinline__ float adam_pick(unsigned bits, int j, float fresh, float old) { return (bits >> j) & 1u ? fresh : old; }

template <bool MASKED>
__global__ __launch_bounds__(kAdamBlock) void k_adam_step(u64 total, u32 w, float *__restrict__ p, const float *__restrict__ g,
                                                          float *__restrict__ m, float *__restrict__ v,
                                                          const uint8_t *__restrict__ visible, AdamScalars S)
{
    const bool narrow = total <= 0xFFFFFFFFull;
    const u64 n4 = total / 4;
    constexpr u64 kTile = (u64)kAdamBatch * kAdamBlock;
    const u64 tiles = (n4 + kTile - 1) / kTile;
    for (u64 t = blockIdx.x; t < tiles; t += gridDim.x) {
        const u64 q0 = t * kTile + threadIdx.x;
        unsigned bits[kAdamBatch];
        float4 P[kAdamBatch], G[kAdamBatch], M[kAdamBatch], V[kAdamBatch];
#pragma unroll
        for (int b = 0; b < kAdamBatch; ++b) {
            const u64 q = q0 + (u64)b * kAdamBlock;
            bits[b] = q < n4 ? (MASKED ? adam_chunk_mask(visible, q, w, narrow) : 0xFu) : 0u;
        }
#pragma unroll
        for (int b = 0; b < kAdamBatch; ++b) {
            const u64 e = 4 * (q0 + (u64)b * kAdamBlock);
            if (bits[b]) {
                P[b] = *reinterpret_cast<const float4 *>(p + e);
                G[b] = *reinterpret_cast<const float4 *>(g + e);
                M[b] = *reinterpret_cast<const float4 *>(m + e);
                V[b] = *reinterpret_cast<const float4 *>(v + e);
            }
        }
#pragma unroll
        for (int b = 0; b < kAdamBatch; ++b) {
            if (!bits[b])
                continue;
            const u64 e = 4 * (q0 + (u64)b * kAdamBlock);
            float4 p1 = P[b], m1 = M[b], v1 = V[b];
            adam_element(p1.x, G[b].x, m1.x, v1.x, S);
            adam_element(p1.y, G[b].y, m1.y, v1.y, S);
            adam_element(p1.z, G[b].z, m1.z, v1.z, S);
            adam_element(p1.w, G[b].w, m1.w, v1.w, S);
            if (MASKED && bits[b] != 0xFu) { // a chunk that straddles a visible and an invisible row: the invisible elements' own bits
                const unsigned k = bits[b];
                p1 = make_float4(adam_pick(k, 0, p1.x, P[b].x), adam_pick(k, 1, p1.y, P[b].y), adam_pick(k, 2, p1.z, P[b].z),
                                 adam_pick(k, 3, p1.w, P[b].w));
                m1 = make_float4(adam_pick(k, 0, m1.x, M[b].x), adam_pick(k, 1, m1.y, M[b].y), adam_pick(k, 2, m1.z, M[b].z),
                                 adam_pick(k, 3, m1.w, M[b].w));
                v1 = make_float4(adam_pick(k, 0, v1.x, V[b].x), adam_pick(k, 1, v1.y, V[b].y), adam_pick(k, 2, v1.z, V[b].z),
                                 adam_pick(k, 3, v1.w, V[b].w));
            }
            *reinterpret_cast<float4 *>(p + e) = p1;
            *reinterpret_cast<float4 *>(m + e) = m1;
            *reinterpret_cast<float4 *>(v + e) = v1;
        }
    }
    // the elements behind the last whole chunk (n w % 4 of them), one thread each
    const u64 e = 4 * n4 + threadIdx.x;
    if (blockIdx.x == 0 && e < total && (!MASKED || visible[adam_row(e, w, narrow)] != 0)) {
        float p1 = p[e], m1 = m[e], v1 = v[e];
        adam_element(p1, g[e], m1, v1, S);
        p[e] = p1, m[e] = m1, v[e] = v1;
    }
}

} // namespace

int launch_adam_step(int64_t n, int w, float *p, const float *g, float *m, float *v, const uint8_t *visible, float lr_over_bc1,
                     float sqrt_bc2, double b1, double b2, float eps, hipStream_t s)
{
    if (n == 0)
        return GWBP_OK;
    const u64 total = (u64)n * (u64)w;
    const u64 tiles = (total / 4 + (u64)kAdamBatch * kAdamBlock - 1) / ((u64)kAdamBatch * kAdamBlock);
    int n_cu = 0;
    if (int rc = device_cus(&n_cu))
        return rc;
    const u64 cap = (u64)n_cu * kAdamWgsPerCu;
    const unsigned grid = (unsigned)(tiles < 1 ? 1 : tiles < cap ? tiles : cap); // (at least workgroup 0: it owns the last elements)
    const AdamScalars S = AdamScalars::make(lr_over_bc1, sqrt_bc2, b1, b2, eps);
    if (visible)
        hipLaunchKernelGGL(k_adam_step<true>, dim3(grid), dim3(kAdamBlock), 0, s, total, (u32)w, p, g, m, v, visible, S);
    else
        hipLaunchKernelGGL(k_adam_step<false>, dim3(grid), dim3(kAdamBlock), 0, s, total, (u32)w, p, g, m, v, visible, S);
    return check_hip(hipGetLastError(), "adam_step launch");
}

} // namespace gwbp
