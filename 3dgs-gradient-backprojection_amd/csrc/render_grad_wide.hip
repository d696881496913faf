// render_grad_wide.hip -- the geometry half of the blend backward for tables of up to 128 channels: v_g2d alone, the gradient of a
// view's [H, W, D] render and alpha map with respect to the six numbers of each projected record the blend reads.
//
// k_render_px_bwd (render_grad.hip) keeps vo[CH] and S[CH] per pixel and stops at 32 channels.  The channels enter d loss / d alpha of
// a (pixel, record j) pair only through a dot product: with m_j = <c_j, vo> the per-channel sum of (c_j T_j - S_j ra_j) vo is
//     v_al = T_j m_j - ra_j B_j + T_final ra_j va,     B_j = sum over the records k behind j of fac_k m_k,
// so a pixel carries ONE scalar B beside vo[CH]: one FMA per channel and pair.  The table's own gradient is a scatter
// of v_out by the blend weights (gwbp_scatter on the weight store of a wide forward render) and is not computed here: no per-channel
// wave sums, no colour atomics.
//
// Otherwise the kernel is k_render_px_bwd: workgroup = 16x16 tile, thread = pixel; pass 1 replays the forward walk with px_blend.h's
// expressions, T in float64 beside the deciding float32 (and in pass 2 everything behind the dot product); pass 2 walks the list back to front in batches of kDotBatch records whose
// colour rows wait in LDS and are read as broadcast 16-B reads.  The order in which tiles reach a Gaussian's row is not fixed: the sums
// are NOT bit-reproducible from run to run.
#include "gwbp_dev.h"
#include "px_blend.h"

namespace gwbp {

typedef float v2f __attribute__((ext_vector_type(2)));

constexpr int kDotBatch = 64; // records of pass 2 staged per batch (128 channels: 32 KiB of colour rows), and flushed together

// (wave_sum_d, the float64 wave sum on wave_sum's DPP controls, is in gwbp_dev.h)

// exp(-max(sigma, 0)) in float64 to about 1e-10 relative, for sigma up to 80: n = rint(x log2 e), a degree-9 Taylor sum on
// r = x - n ln 2 (|r| <= 0.35: the first term left out is below 1e-11), times 2^n.
__device__ __forceinline__ double exp_neg_d(double sigma)
{
    const double x = -__builtin_fmin(__builtin_fmax(sigma, 0.0), 80.0);
    const double n = __builtin_rint(x * 0x1.71547652b82fep+0);
    const double r = __builtin_fma(n, -0x1.62e42fefa39efp-1, x);
    double p = 1.0 / 362880.0;
    p = __builtin_fma(p, r, 1.0 / 40320.0);
    p = __builtin_fma(p, r, 1.0 / 5040.0);
    p = __builtin_fma(p, r, 1.0 / 720.0);
    p = __builtin_fma(p, r, 1.0 / 120.0);
    p = __builtin_fma(p, r, 1.0 / 24.0);
    p = __builtin_fma(p, r, 1.0 / 6.0);
    p = __builtin_fma(p, r, 0.5);
    p = __builtin_fma(p, r, 1.0);
    p = __builtin_fma(p, r, 1.0);
    return __builtin_ldexp(p, (int)n);
}

// CH = channels held per pixel (64 or 128; D <= CH).  v_g2d [N, 6] is added into; v_alpha [H, W] or nullptr.  Every loop bound is
// workgroup-uniform, every skip inside the record loops is wave-uniform (ballots) and lies between barriers, never around one; pixels
// outside the image walk along with done / live = false.
template <int CH>
__global__ __launch_bounds__(256, 2) void k_render_dots_bwd(ViewDev V, const u32 *__restrict__ tile_offsets,
                                                         const u32 *__restrict__ vals, const G2D *__restrict__ g2d,
                                                         const float *__restrict__ colors, int64_t ldc, int D,
                                                         const float *__restrict__ v_out, const float *__restrict__ v_alpha,
                                                         float *__restrict__ v_g2d)
{
    __shared__ float4 s_a[256]; // mx, my, opac, ln(255 opac) + margin (pass 1: 256 records; pass 2: the first kDotBatch)
    __shared__ float4 s_b[256]; // ca, cb, cc, -
    __shared__ float4 s_c[kDotBatch][CH / 4]; // colour rows, zero behind D
    __shared__ u32 s_gid[kDotBatch];
    __shared__ double s_part[4][kDotBatch][6]; // [wave][record of the batch][value]; all zero between two flushes
    __shared__ u32 s_last;
    const int tile = blockIdx.x;
    const int tx = tile % V.tile_w, ty = tile / V.tile_w;
    const int lane = threadIdx.x & 63;
    const int wave = (int)uniform(threadIdx.x >> 6);
    const int ix = tx * kTile + (lane & 15), iy = ty * kTile + wave * 4 + (lane >> 4);
    const bool inside = ix < V.W && iy < V.H;
    const float px = (float)ix + 0.5f, py = (float)iy + 0.5f;
    const u32 beg = tile_offsets[tile], end = tile_offsets[tile + 1];
    for (int i = threadIdx.x; i < 4 * kDotBatch * 6; i += 256)
        (&s_part[0][0][0])[i] = 0.0;
    if (threadIdx.x == 0)
        s_last = 0u;
    __syncthreads();

    // ---- pass 1: k_render_px's walk without the colours -> T after the last record, and that record's position + 1 ----
    float T = 1.0f;
    bool done = !inside;
    u32 last = 0u; // position (from beg) of the pixel's last contributing record, plus one; 0: none
    double Td = 1.0; // the same product in float64, beside the float32 T that decides (render_grad.hip)
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
    const double T_final = Td;
    const size_t pix = (size_t)iy * V.W + ix;
    v2f vo[CH / 2]; // d loss / d out of this pixel, in the pairs the packed FMAs read
    if ((D & 3) == 0 && (reinterpret_cast<uintptr_t>(v_out) & 15) == 0) { // (uniform: kernel arguments) the row in 16-B loads
        const float4 *vp = reinterpret_cast<const float4 *>(v_out + pix * D);
#pragma unroll
        for (int c4 = 0; c4 < CH / 4; ++c4) {
            const float4 q = (inside && 4 * c4 < D) ? vp[c4] : make_float4(0.f, 0.f, 0.f, 0.f);
            vo[2 * c4] = v2f{q.x, q.y}, vo[2 * c4 + 1] = v2f{q.z, q.w};
        }
    } else {
#pragma unroll
        for (int c = 0; c < CH; c += 2)
            vo[c / 2] = v2f{(inside && c < D) ? v_out[pix * D + c] : 0.f, (inside && c + 1 < D) ? v_out[pix * D + c + 1] : 0.f};
    }
    const float va = (inside && v_alpha) ? v_alpha[pix] : 0.f;
    double B = 0.0; // sum of fac_k m_k over the records behind the current one
    for (u32 bi = (n_used + kDotBatch - 1u) / kDotBatch; bi-- > 0u;) {
        const u32 base = bi * kDotBatch;
        const u32 bn = min((u32)kDotBatch, n_used - base);
        // (the barrier behind the last flush, or the one behind s_last, separates this staging from every earlier read)
        if (threadIdx.x < bn) {
            const u32 gid = vals[beg + base + threadIdx.x];
            const float4 *gp = reinterpret_cast<const float4 *>(g2d + gid);
            s_a[threadIdx.x] = px_stage(gp[0]);
            s_b[threadIdx.x] = gp[1];
            s_gid[threadIdx.x] = gid;
        }
        __syncthreads();
        // the rows: thread -> (record, channel) with the channel fastest, so a wave reads 64 consecutive floats of one row
        for (u32 i = threadIdx.x; i < bn * (u32)CH; i += 256u) {
            const u32 r = i / (u32)CH, c = i % (u32)CH; // (CH is a power of two: a shift and a mask)
            (&s_c[0][0].x)[i] = (int)c < D ? colors[(int64_t)s_gid[r] * ldc + c] : 0.f;
        }
        __syncthreads();
        for (u32 j = bn; j-- > 0u;) {
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
            // m = <c_j, vo> with exact products and float64 sums, in four chains (one per component of the 16-B read).  A float32
            // dot product leaves about sqrt(D) roundings of its partial sums in m; the sums over a record's pixels cancel (dx dy changes
            // sign across the record), and what is left of those roundings, bare on a one-record list, was 15 x the float32
            // reference's error in the cb column.  Two conversions and one float64 FMA per channel and pair.
            double md[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int c4 = 0; c4 < CH / 4; ++c4) {
                const float4 c = s_c[j][c4];
                // (vo is loop-invariant and its 128 conversions would be hoisted out of the record loop into 256 registers: the empty
                // statements make each pair opaque here, so that it is converted where it is used)
                asm volatile("" : "+v"(vo[2 * c4]), "+v"(vo[2 * c4 + 1]));
                md[0] = __builtin_fma((double)c.x, (double)vo[2 * c4].x, md[0]);
                md[1] = __builtin_fma((double)c.y, (double)vo[2 * c4].y, md[1]);
                md[2] = __builtin_fma((double)c.z, (double)vo[2 * c4 + 1].x, md[2]);
                md[3] = __builtin_fma((double)c.w, (double)vo[2 * c4 + 1].y, md[3]);
            }
            const double rad = 1.0 / (1.0 - (double)alpha);
            const double Tjd = Td * rad; // T in front of this record
            Td = valid ? Tjd : Td;
            const double m = (md[0] + md[2]) + (md[1] + md[3]);
            // Behind the dot product everything is float64 up to the one rounding in front of the atomic: T_j m_j and ra_j B_j cancel,
            // ca dx + cb dy cancels, and a record's 256 terms cancel again in the sums over the pixels -- in float32 each of these left
            // its rounding, magnified by the cancellation, in a sum that the one-record list shows bare.  Per pair, not per channel.
            double v_al = __builtin_fma(Tjd, m, -(rad * B));
            v_al = __builtin_fma(T_final * rad, (double)va, v_al);
            // the pair's own factors once more in float64, from the same float32 record: the float32 sigma carries half an ulp of its
            // size (up to 5.5) as a RELATIVE error into exp(-sigma), and exp_neg another ulp; which pairs count, the clamp and T stay
            // with the float32 alpha, as the forward decided them
            const double dx = (double)a.x - (double)px, dy = (double)a.y - (double)py;
            const double sigma_d = __builtin_fma((double)b.y * dx, dy, 0.5 * __builtin_fma((double)b.x * dx, dx, ((double)b.z * dy) * dy));
            const double vis_d = exp_neg_d(sigma_d);
            const double raw_d = (double)a.z * vis_d;
            // (selects, not products with 0: a non-finite colour must reach only the pairs that are valid)
            const bool moves = valid && raw <= kAlphaMax; // a clamped alpha does not depend on the geometry or the opacity
            B = valid ? __builtin_fma((moves ? raw_d : (double)alpha) * Tjd, m, B) : B;
            const double v_sigma = moves ? -(raw_d * v_al) : 0.0;
            const double sx = v_sigma * dx, sy = v_sigma * dy;
            double mine = 0.0; // lane v keeps the wave's sum of value v
            // one value at a time, each summed before the next is formed (the scheduling barrier keeps six doubles and their DPP
            // temporaries from being live beside vo[CH]: the 128-channel instantiation has no register to spare)
#define GWBP_DOT_SUM(V, EXPR)                                                                                                      \
    {                                                                                                                              \
        const double r = wave_sum_d(EXPR);                                                                                         \
        mine = lane == (V) ? r : mine;                                                                                             \
        __builtin_amdgcn_sched_barrier(0);                                                                                         \
    }
            GWBP_DOT_SUM(0, __builtin_fma((double)b.x, sx, (double)b.y * sy))
            GWBP_DOT_SUM(1, __builtin_fma((double)b.y, sx, (double)b.z * sy))
            GWBP_DOT_SUM(2, 0.5 * sx * dx)
            GWBP_DOT_SUM(3, sx * dy)
            GWBP_DOT_SUM(4, 0.5 * sy * dy)
            GWBP_DOT_SUM(5, moves ? vis_d * v_al : 0.0)
#undef GWBP_DOT_SUM
            if (lane < 6)
                s_part[wave][j][lane] = mine;
        }
        __syncthreads();
        // the batch's sums: the four waves' partials in wave order, one atomic per value that is not zero
        for (u32 i = threadIdx.x; i < (u32)(kDotBatch * 6); i += 256u) {
            const u32 r = i / 6u, v = i % 6u;
            const float sum = (float)(((s_part[0][r][v] + s_part[1][r][v]) + s_part[2][r][v]) + s_part[3][r][v]);
            s_part[0][r][v] = s_part[1][r][v] = s_part[2][r][v] = s_part[3][r][v] = 0.0;
            if (r < bn && sum != 0.f)
                atomicAdd(v_g2d + (size_t)s_gid[r] * 6u + v, sum);
        }
        __syncthreads();
    }
}

int launch_render_dots_bwd(const Ws &W, const ViewDev &V, const float *colors, int64_t ldc, int D, const float *v_out,
                           const float *v_alpha, float *v_g2d, hipStream_t s)
{
    const int n_tiles = V.tile_w * V.tile_h;
    const int fin = sort_passes(n_tiles) & 1;
#define GWBP_DOTB(C)                                                                                                                \
    hipLaunchKernelGGL((k_render_dots_bwd<C>), dim3(n_tiles), dim3(256), 0, s, V, W.tile_offsets, W.vals[fin], W.g2d, colors, ldc, D, \
                       v_out, v_alpha, v_g2d)
    if (D <= 64)
        GWBP_DOTB(64);
    else
        GWBP_DOTB(128);
#undef GWBP_DOTB
    return check_hip(hipGetLastError(), "render_dots_bwd launch");
}

} // namespace gwbp
