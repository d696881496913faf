// pixels.hip -- which Gaussians a pixel is made of: the k contributing records of largest weight w = alpha * T per pixel, the number of
// contributing records, alpha, and the record at which T falls to one half (its id and camera depth: the median depth).  Needs only
// project + bin_sort of the view, like k_render_px; reads the workspace and writes nothing into it.
//
//   RESULT per pixel: the k contributing records of largest weight by (w descending, Gaussian id ascending); ids tail -1, weights tail
//     0; n_contrib = the number of contributing records (> k: the list was cut); alpha = 1 - T; median = the first contributing
//     record, in list order, after which T <= 0.5 (-1 and depth 0 where T stays above one half).
// A tile list holds a Gaussian once, so a pixel's list is the top k of a SET under a total order: the result does not depend on how
// the list is kept, which is what makes the two kernels below equal bit for bit.
//
// k_pixel_gaussians: the image form, k_render_px's walk (render.hip) -- workgroup = 16x16 tile, thread = pixel, records staged in LDS
//   per batch of 256, the blend step of px_blend.h, the same two wave-uniform early-outs and batch exit -- with a
//   LaneTopK<HeaviestFirst> (lane_topk.h) in dynamic LDS in place of the colour accumulators: k * 256 * 8 bytes <= 32 KiB.  The record's
//   Gaussian id and camera depth are staged beside its two float4s.  The insert is lane-divergent LDS traffic in lane-private
//   columns: no barrier inside it, and every loop that holds a barrier or a ballot stays workgroup- or wave-uniform.
// k_pixel_gaussians_at: the pixel-list form, k_probe_pixels' walk (query_kernel.h) -- one wave per pixel, lanes = list entries for
//   sigma and alpha, T advanced entry by entry in list order with wave-uniform values.  The running list lives one entry per lane in
//   lanes 0..k-1: an insert finds its position by a ballot of "orders before" and shifts the lanes behind it by one.
#include "gwbp_dev.h"
#include "lane_topk.h"
#include "px_blend.h"

namespace gwbp {

namespace {

constexpr float kMedianT = 0.5f;

__global__ __launch_bounds__(256) void k_pixel_gaussians(ViewDev V, const u32 *__restrict__ tile_offsets, const u32 *__restrict__ vals,
                                                         const G2D *__restrict__ g2d, int k, int32_t *__restrict__ ids,
                                                         float *__restrict__ weights, int32_t *__restrict__ n_contrib,
                                                         float *__restrict__ alphas, int32_t *__restrict__ median_id,
                                                         float *__restrict__ median_depth)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ float4 s_a[256]; // mx, my, opac, ln(255 opac) + margin
    __shared__ float4 s_b[256]; // ca, cb, cc, -
    __shared__ int s_gid[256];
    __shared__ float s_z[256];  // the camera depth px_stage overwrites
    LaneTopK<HeaviestFirst, 256> best(smem, k, threadIdx.x);
    const int tile = blockIdx.x;
    const int tx = tile % V.tile_w, ty = tile / V.tile_w;
    const int lane = threadIdx.x & 63;
    const int wave = (int)uniform(threadIdx.x >> 6);
    const int ix = tx * kTile + (lane & 15), iy = ty * kTile + wave * 4 + (lane >> 4);
    const bool inside = ix < V.W && iy < V.H;
    const float px = (float)ix + 0.5f, py = (float)iy + 0.5f;
    const u32 beg = tile_offsets[tile], end = tile_offsets[tile + 1];
    float T = 1.0f;
    bool done = !inside;
    int nc = 0, med = -1;
    float med_z = 0.f;
    best.init();
    for (u32 batch = beg; batch < end; batch += 256) {
        if (__syncthreads_count(done) == 256)
            break;
        const u32 bn = min(256u, end - batch);
        if (threadIdx.x < bn) {
            const u32 gid = vals[batch + threadIdx.x];
            const float4 *gp = reinterpret_cast<const float4 *>(g2d + gid);
            const float4 a = gp[0];
            s_a[threadIdx.x] = px_stage(a);
            s_b[threadIdx.x] = gp[1];
            s_gid[threadIdx.x] = (int)gid;
            s_z[threadIdx.x] = a.w;
        }
        __syncthreads();
        for (u32 j = 0; j < bn; ++j) {
            if (__ballot(!done) == 0ull)
                break;
            const float4 a = s_a[j], b = s_b[j];
            const float sigma = px_sigma(a, b, px, py);
            if (px_quarter_outside(done, sigma, a.w))
                continue; // no live pixel of this quarter inside the alpha >= 1/255 ellipse
            float w;
            const bool valid = px_step(sigma, a.z, T, done, w);
            if (px_nobody(valid))
                continue; // nobody lists this Gaussian
            if (valid) { // lane-divergent from here to the end of the body: no barrier, no ballot
                const int gid = s_gid[j];
                ++nc;
                best.offer(w, gid);
                if (med < 0 && T <= kMedianT) {
                    med = gid;
                    med_z = s_z[j];
                }
            }
        }
    }
    if (inside) {
        const size_t p = (size_t)iy * V.W + ix;
        for (int j = 0; j < k; ++j) {
            ids[p * k + j] = best.index(j);
            weights[p * k + j] = best.key(j); // (0 in an empty slot)
        }
        if (n_contrib)
            n_contrib[p] = nc;
        if (alphas)
            alphas[p] = 1.0f - T;
        if (median_id)
            median_id[p] = med;
        if (median_depth)
            median_depth[p] = med_z;
    }
}

__device__ __forceinline__ float bcast_f(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ float from_lane_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

__global__ __launch_bounds__(64) void k_pixel_gaussians_at(ViewDev V, const u32 *__restrict__ tile_offsets, const u32 *__restrict__ vals,
                                                           const G2D *__restrict__ g2d, const int32_t *__restrict__ xy, int k,
                                                           int32_t *__restrict__ ids, float *__restrict__ weights,
                                                           int32_t *__restrict__ n_contrib, float *__restrict__ alphas,
                                                           int32_t *__restrict__ median_id, float *__restrict__ median_depth)
{
    const int m = (int)blockIdx.x;
    const int lane = threadIdx.x;
    const int ix = (int)uniform((u32)xy[2 * m]), iy = (int)uniform((u32)xy[2 * m + 1]);
    const bool inside = ix >= 0 && ix < V.W && iy >= 0 && iy < V.H;
    const u64 list_lanes = (1ull << k) - 1ull; // k <= 16

    float my_w = HeaviestFirst::empty(); // entry `lane` of the list, lanes 0..k-1
    int my_id = kNoIndex;
    float T = 1.0f, med_z = 0.f;
    int nc = 0, med = -1;
    if (inside) { // wave-uniform
        const int tile = (iy / kTile) * V.tile_w + ix / kTile;
        const u32 beg = uniform(tile_offsets[tile]), end = uniform(tile_offsets[tile + 1]);
        const float px = (float)ix + 0.5f, py = (float)iy + 0.5f;
        bool done = false;
        for (u32 batch = beg; batch < end && !done; batch += 64) {
            const u32 bn = min(64u, end - batch);
            u32 gid = 0;
            float alpha = 0.f, z = 0.f;
            bool ok = false;
            if ((u32)lane < bn) {
                gid = vals[batch + lane];
                const float4 *gp = reinterpret_cast<const float4 *>(g2d + gid);
                const float4 a = gp[0], b = gp[1];
                const float sigma = px_sigma(a, b, px, py);
                alpha = __builtin_fminf(kAlphaMax, a.z * exp_neg(-__builtin_fmaxf(sigma, 0.f)));
                ok = (sigma >= 0.f) && (alpha >= kAlphaMin);
                z = a.w;
            }
            const u64 okm = __ballot(ok);
            // T through the batch in list order: every value below is wave-uniform
            for (u32 j = 0; j < bn; ++j) {
                if (!((okm >> j) & 1ull))
                    continue;
                const float al = from_lane_f(alpha, (int)j);
                const float next_T = bcast_f(T * (1.0f - al));
                if (next_T <= kTMin) { // terminates: not counted, nothing behind it either
                    done = true;
                    break;
                }
                const float w = bcast_f(al * T);
                const int g = __builtin_amdgcn_readlane((int)gid, (int)j);
                T = next_T;
                ++nc;
                if (med < 0 && T <= kMedianT) {
                    med = g;
                    med_z = from_lane_f(z, (int)j);
                }
                // the entries that order before (w, g) are a prefix of the sorted list: their count is the new entry's position
                const bool before = HeaviestFirst::first(my_w, w) || (my_w == w && my_id < g);
                const int pos = __popcll(__ballot(before) & list_lanes);
                if (pos < k) {
                    const float up_w = __shfl_up(my_w, 1, 64);
                    const int up_id = __shfl_up(my_id, 1, 64);
                    if (lane > pos) {
                        my_w = up_w;
                        my_id = up_id;
                    }
                    if (lane == pos) {
                        my_w = w;
                        my_id = g;
                    }
                }
            }
        }
    }
    if (lane < k) {
        ids[(int64_t)m * k + lane] = my_id == kNoIndex ? -1 : my_id;
        weights[(int64_t)m * k + lane] = my_w; // (0 in an empty slot)
    }
    if (lane == 0) {
        if (n_contrib)
            n_contrib[m] = nc;
        if (alphas)
            alphas[m] = 1.0f - T;
        if (median_id)
            median_id[m] = med;
        if (median_depth)
            median_depth[m] = med_z;
    }
}

} // namespace

int launch_pixel_gaussians(const Ws &W, const ViewDev &V, int k, int M, const int32_t *xy, int32_t *ids, float *weights,
                           int32_t *n_contrib, float *alphas, int32_t *median_id, float *median_depth, hipStream_t s)
{
    const int n_tiles = V.tile_w * V.tile_h;
    const int fin = sort_passes(n_tiles) & 1;
    if (xy) {
        hipLaunchKernelGGL(k_pixel_gaussians_at, dim3((unsigned)M), dim3(64), 0, s, V, W.tile_offsets, W.vals[fin], W.g2d, xy, k, ids,
                           weights, n_contrib, alphas, median_id, median_depth);
    } else {
        const size_t lds = lane_columns_bytes(k, 256); // <= 32 KiB + 10 KiB of staging: below the default limit
        hipLaunchKernelGGL(k_pixel_gaussians, dim3(n_tiles), dim3(256), lds, s, V, W.tile_offsets, W.vals[fin], W.g2d, k, ids, weights,
                           n_contrib, alphas, median_id, median_depth);
    }
    return check_hip(hipGetLastError(), "pixel_gaussians launch");
}

} // namespace gwbp
