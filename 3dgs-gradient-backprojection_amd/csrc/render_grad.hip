// render_grad.hip -- backward of the pixel-parallel render (k_render_px, render.hip): the gradient of a view's [H, W, D] render and
// alpha map with respect to the colour table and to the six numbers of each projected record the blend reads.
//
// gsplat's rasterize_to_pixels_bwd, on this project's tile lists: workgroup = 16x16 tile, thread = pixel, records staged in LDS in
// batches of 256.  Pass 1 replays the forward walk with px_blend.h's expressions (the same bits as the render: each pixel's final T and
// the list position of its last contributing record); pass 2 walks the list back to front, recovers T by division, and adds each
// record's gradient -- summed over the wave, then over the four waves in wave order through LDS -- with one global float atomic per
// value.  The chain rule through the projection is N-sized and not done here (projection.py).
//
// The order in which tiles reach a Gaussian's row is not fixed: the sums are NOT bit-reproducible from run to run.
#include "gwbp_dev.h"
#include "px_blend.h"

namespace gwbp {

constexpr int kGradSub = 32; // records whose per-wave partial sums wait in LDS between two flushes

// CH = channels held per pixel (4, 16 or 32; D <= CH).  v_g2d [N, 6] = d / d(mx, my, ca, cb, cc, o), o the filed opacity (already
// times the antialiasing compensation); v_colors [N, D] or nullptr; v_alpha [H, W] or nullptr.  Both outputs are added into.
// Every loop bound is workgroup-uniform (tile_offsets, and the largest last position of the tile's pixels, read from LDS behind a
// barrier); every skip inside the record loops is wave-uniform (ballots) and lies between barriers, never around one; pixels outside the
// image walk along with done / live = false.
template <int CH>
__global__ __launch_bounds__(256) void k_render_px_bwd(ViewDev V, const u32 *__restrict__ tile_offsets,
                                                       const u32 *__restrict__ vals, const G2D *__restrict__ g2d,
                                                       const float *__restrict__ colors, int64_t ldc, int D,
                                                       const float *__restrict__ v_out, const float *__restrict__ v_alpha,
                                                       float *__restrict__ v_colors, float *__restrict__ v_g2d)
{
    constexpr int NV = 6 + CH; // values per record: the six of the G2D record, then the colours
    __shared__ float4 s_a[256]; // mx, my, opac, ln(255 opac) + margin
    __shared__ float4 s_b[256]; // ca, cb, cc, -
    __shared__ float4 s_c[256][CH / 4]; // colour
    __shared__ u32 s_gid[256];
    __shared__ float s_part[4][kGradSub][NV]; // [wave][record of the sub-batch][value]; all zero between two flushes
    __shared__ u32 s_last;
    const int tile = blockIdx.x;
    const int tx = tile % V.tile_w, ty = tile / V.tile_w;
    const int lane = threadIdx.x & 63;
    const int wave = (int)uniform(threadIdx.x >> 6);
    const int ix = tx * kTile + (lane & 15), iy = ty * kTile + wave * 4 + (lane >> 4);
    const bool inside = ix < V.W && iy < V.H;
    const float px = (float)ix + 0.5f, py = (float)iy + 0.5f;
    const u32 beg = tile_offsets[tile], end = tile_offsets[tile + 1];
    for (int i = threadIdx.x; i < 4 * kGradSub * NV; i += 256)
        (&s_part[0][0][0])[i] = 0.f;
    if (threadIdx.x == 0)
        s_last = 0u;
    __syncthreads();

    // ---- pass 1: k_render_px's walk without the colours -> T after the last record, and that record's position + 1 ----
    float T = 1.0f;
    bool done = !inside;
    u32 last = 0u; // position (from beg) of the pixel's last contributing record, plus one; 0: none
    // The same product once more in float64, beside the float32 T that decides (and is never read from here): pass 2 divides its way
    // back through up to the whole list, and in float32 every step of both walks would leave its rounding in the T of the records in
    // front, which weigh most.  Two float64 operations per pair.
    double Td = 1.0;
    for (u32 batch = beg; batch < end; batch += 256) {
        if (__syncthreads_count(done) == 256)
            break;
        const u32 bn = min(256u, end - batch);
        if (threadIdx.x < bn) {
            const float4 *gp = reinterpret_cast<const float4 *>(g2d + vals[batch + threadIdx.x]);
            s_a[threadIdx.x] = px_stage(gp[0]);
            s_b[threadIdx.x] = gp[1];
        }
        __syncthreads();
        for (u32 j = 0; j < bn; ++j) {
            if (__ballot(!done) == 0ull)
                break;
            const float4 a = s_a[j], b = s_b[j];
            const float sigma = px_sigma(a, b, px, py);
            if (px_quarter_outside(done, sigma, a.w))
                continue;
            float w, vis, raw;
            const float alpha = px_alpha(sigma, a.z, vis, raw); // (px_step's own expression: one evaluation)
            const bool valid = px_step(sigma, a.z, T, done, w);
            last = valid ? batch - beg + j + 1u : last;
            Td = valid ? Td * (1.0 - (double)alpha) : Td;
        }
    }
    atomicMax(&s_last, last);
    __syncthreads();
    const u32 n_used = s_last; // records of the tile's list up to the last one any of its pixels took
    if (n_used == 0u)
        return; // (the whole workgroup: nobody contributes to this tile)

    // ---- pass 2: back to front ----
    const float T_final = (float)Td;
    const size_t pix = (size_t)iy * V.W + ix;
    float vo[CH], S[CH]; // d loss / d out of this pixel; colour accumulated behind the current record
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        vo[c] = (inside && c < D) ? v_out[pix * D + c] : 0.f;
        S[c] = 0.f;
    }
    const float va = (inside && v_alpha) ? v_alpha[pix] : 0.f;
    const bool want_colors = v_colors != nullptr;
    for (u32 bi = (n_used + 255u) / 256u; bi-- > 0u;) {
        const u32 base = bi * 256u;
        const u32 bn = min(256u, n_used - base);
        // (the barrier behind the last flush, or the one behind s_last, separates this staging from every earlier read)
        if (threadIdx.x < bn) {
            const u32 gid = vals[beg + base + threadIdx.x];
            const float4 *gp = reinterpret_cast<const float4 *>(g2d + gid);
            s_a[threadIdx.x] = px_stage(gp[0]);
            s_b[threadIdx.x] = gp[1];
            s_gid[threadIdx.x] = gid;
            const float *cp = colors + (int64_t)gid * ldc;
            float cv[CH];
#pragma unroll
            for (int c = 0; c < CH; ++c)
                cv[c] = c < D ? cp[c] : 0.f;
#pragma unroll
            for (int c4 = 0; c4 < CH / 4; ++c4)
                s_c[threadIdx.x][c4] = make_float4(cv[4 * c4], cv[4 * c4 + 1], cv[4 * c4 + 2], cv[4 * c4 + 3]);
        }
        __syncthreads();
        for (u32 sb = (bn + kGradSub - 1u) / kGradSub; sb-- > 0u;) {
            const u32 j0 = sb * kGradSub, j1 = min(bn, j0 + kGradSub);
            for (u32 j = j1; j-- > j0;) {
                const float4 a = s_a[j], b = s_b[j];
                const bool live = base + j < last; // at or before the pixel's last record: the forward's !done
                const float sigma = px_sigma(a, b, px, py);
                if (px_quarter_outside(!live, sigma, a.w))
                    continue;
                float vis, raw;
                const float alpha = px_alpha(sigma, a.z, vis, raw);
                const bool valid = live && (sigma >= 0.f) && (alpha >= kAlphaMin); // exactly the forward's valid pairs
                if (px_nobody(valid))
                    continue;
                const float ra = 1.0f / (1.0f - alpha);
                const double Tjd = Td / (1.0 - (double)alpha); // T in front of this record
                Td = valid ? Tjd : Td;
                const float Tj = (float)Tjd;
                const float fac = alpha * Tj;
                float mine = 0.f; // lane v keeps the wave's sum of value v
                float v_al = 0.f; // d loss / d alpha of this pair
#pragma unroll
                for (int c4 = 0; c4 < CH / 4; ++c4) {
                    const float4 c = s_c[j][c4];
                    const float cc[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int ch = 4 * c4 + k;
                        v_al = __builtin_fmaf(cc[k] * Tj - S[ch] * ra, vo[ch], v_al);
                        S[ch] = valid ? __builtin_fmaf(cc[k], fac, S[ch]) : S[ch];
                        if (want_colors && ch < D) { // (uniform: kernel arguments)
                            const float r = wave_sum(valid ? fac * vo[ch] : 0.f);
                            mine = lane == 6 + ch ? r : mine;
                        }
                    }
                }
                v_al = __builtin_fmaf(T_final * ra, va, v_al);
                // (selects, not products with 0: a non-finite colour must reach only the pairs that are valid)
                const bool moves = valid && raw <= kAlphaMax; // a clamped alpha does not depend on the geometry or the opacity
                const float v_sigma = moves ? -(raw * v_al) : 0.f;
                const float dx = a.x - px, dy = a.y - py;
                const float g[6] = {v_sigma * (b.x * dx + b.y * dy), v_sigma * (b.y * dx + b.z * dy), 0.5f * v_sigma * dx * dx,
                                    v_sigma * dx * dy,               0.5f * v_sigma * dy * dy,          moves ? vis * v_al : 0.f};
#pragma unroll
                for (int v = 0; v < 6; ++v) {
                    const float r = wave_sum(g[v]);
                    mine = lane == v ? r : mine;
                }
                if (lane < NV)
                    s_part[wave][j - j0][lane] = mine;
            }
            __syncthreads();
            // the sub-batch's sums: the four waves' partials in wave order, one atomic per value that is not zero
            const u32 cnt = j1 - j0;
            for (u32 i = threadIdx.x; i < (u32)(kGradSub * NV); i += 256u) {
                const u32 r = i / NV, v = i % NV;
                const float sum = ((s_part[0][r][v] + s_part[1][r][v]) + s_part[2][r][v]) + s_part[3][r][v];
                s_part[0][r][v] = s_part[1][r][v] = s_part[2][r][v] = s_part[3][r][v] = 0.f;
                if (r < cnt && sum != 0.f) {
                    const size_t gid = s_gid[j0 + r];
                    if (v < 6u)
                        atomicAdd(v_g2d + gid * 6u + v, sum);
                    else if (want_colors && (int)(v - 6u) < D)
                        atomicAdd(v_colors + gid * (size_t)D + (v - 6u), sum);
                }
            }
            __syncthreads();
        }
    }
}

int launch_render_px_bwd(const Ws &W, const ViewDev &V, const float *colors, int64_t ldc, int D, const float *v_out,
                         const float *v_alpha, float *v_colors, float *v_g2d, hipStream_t s)
{
    const int n_tiles = V.tile_w * V.tile_h;
    const int fin = sort_passes(n_tiles) & 1;
#define GWBP_PXB(C)                                                                                                               \
    hipLaunchKernelGGL((k_render_px_bwd<C>), dim3(n_tiles), dim3(256), 0, s, V, W.tile_offsets, W.vals[fin], W.g2d, colors, ldc, D, \
                       v_out, v_alpha, v_colors, v_g2d)
    if (D <= 4)
        GWBP_PXB(4);
    else if (D <= 16)
        GWBP_PXB(16);
    else
        GWBP_PXB(32);
#undef GWBP_PXB
    return check_hip(hipGetLastError(), "render_px_bwd launch");
}

} // namespace gwbp
