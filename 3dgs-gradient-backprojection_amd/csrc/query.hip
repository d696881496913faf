// query.hip -- questions asked of a finished [N, D] feature field (the reference's segment.py / segment_compressed.py /
// click_and_segment.py: get_mask3d_lseg, and the render of the field that the click script reads one pixel of):
//
//   k_prompt_scores   s[g, j] = X[g] . prompts[j] (/ max(|X[g]|, 1e-12)),  j < P <= 32, and the 3-D mask
//                     max_{j < n_pos} s[g, j] > max_{j >= n_pos} s[g, j]  (&& s[g, 0] > threshold): ONE pass over X
//   k_probe_pixels    out[m, :] = sum_g w_g(p_m) X[g, :] at M pixels only, + the accumulated depth and alpha of those pixels
//
// k_prompt_scores itself is query_kernel.h, a template over the element type of X: this file instantiates it for fp32 fields,
// query_half.hip for fp16 / bf16 ones (widened exactly as they are loaded: the same staged values, chains and results).
//
// ARITHMETIC CONTRACT of k_prompt_scores (the shape of k_pca_project's, pca.hip).  Every dot product AND the row's sum of squares
// is one chain of fp32 fused multiply-adds over the channel index (v_mfma_f32_16x16x4_f32 is bit for bit a k-ordered fmaf chain; the
// sum of squares is the diagonal of the row block's own 16 x 16 product, so it runs through the columns in the very order of the
// dot products), in an order that depends only on D: every chain consumes k = 32 c + 16 b + 4 q + i in the order (c, b, i, q) --
// the 32-column chunk staged per step, its 16-column block, the float4 component that feeds one MFMA, the quarter wave (the MFMA's
// k slot) -- which is knn_tile.h's order.  Columns D .. 32 ceil(D / 32) - 1 are zero-filled in LDS and their steps are executed
// (fmaf(0, 0, acc) == acc, but -0 becomes +0).  The norm is one correctly rounded sqrt, the score one correctly rounded
// divide.  Nothing depends on the row's position, on N, on P (the 16 prompts of a block are independent output columns) or on the
// launch; rows whose address and stride are 16-B aligned are read with 16-B loads, others element by element: same values, same
// chains.  Padding beyond D is never read (load4 masks it).  No atomics.  The two maxima propagate NaN as torch.max does, so a NaN
// score loses the comparison whichever side it is on.
//
// WHY NOT pca.hip's STAGING CODE.  k_pca_project subtracts the mean while it stages, stages one 16-row operand block and ends in a
// min / max reduction; here nothing is subtracted, one or two 16-prompt blocks are staged and the row block is its own second
// operand.  One shared staging routine would need a flag for the subtraction and another for the operand count inside the loop
// that decides both kernels' speed; the forty lines are kept apart and k_pca_project is not touched (its output is pinned bit for
// bit by its tests).  The prompts are staged chunk by chunk beside X (32 prompts x 2048 channels do not fit LDS at once); they
// are 256 KB at most and stay in L2.
//
// k_probe_pixels is not a second render path: it walks ONE pixel's tile list with the expressions of k_render_px (render.hip) /
// k_blend -- same sigma, exp_neg, kAlphaMin / kAlphaMax / kTMin cuts -- so its weights are the blend's bit for bit, and adds
// acc[c] = fmaf(w, X[g, c], acc[c]) front to back, the per-pixel order of k_render_px and of k_render_rows (render_wide.hip: "every
// pixel is summed front to back by its one owner").  Every loop is wave-uniform with a finite trip count (list batches, 64
// entries of a batch, the set bits of a 64-bit mask); T advances on values made uniform with v_readfirstlane.
#include "gwbp_dev.h"
#include "query_kernel.h"

namespace gwbp {

namespace {

// ---- probe ----------------------------------------------------------------------------------------------------------------------
constexpr int kProbeChunk = 256; // channels per wave: four per lane

__device__ __forceinline__ float uniform_f(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ float lane_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// One wave per (probe, 256-channel chunk).  Per batch of 64 list entries: lanes = entries compute sigma and alpha; the wave then
// advances T entry by entry in list order (uniform values) and leaves each entry's weight in its lane; at last the entries that
// have a weight are added front to back, lanes = channels.
template <bool VEC>
__global__ __launch_bounds__(64) void k_probe_pixels(ViewDev V, const u32 *__restrict__ tile_offsets, const u32 *__restrict__ vals,
                                                     const G2D *__restrict__ g2d, const int32_t *__restrict__ xy,
                                                     const float *__restrict__ X, int64_t ldx, int D, float *__restrict__ out,
                                                     float *__restrict__ depth, float *__restrict__ alpha_out)
{
    const int probe = (int)blockIdx.x, chunk = (int)blockIdx.y;
    const int lane = threadIdx.x;
    const int c = chunk * kProbeChunk + 4 * lane;
    const int ix = (int)uniform((u32)xy[2 * probe]), iy = (int)uniform((u32)xy[2 * probe + 1]);
    const bool inside = ix >= 0 && ix < V.W && iy >= 0 && iy < V.H;

    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float zacc = 0.f, T = 1.0f;
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
                const float dx = a.x - px, dy = a.y - py;
                const float sigma = __builtin_fmaf(b.y * dx, dy, 0.5f * __builtin_fmaf(b.x * dx, dx, (b.z * dy) * dy));
                alpha = __builtin_fminf(kAlphaMax, a.z * exp_neg(-__builtin_fmaxf(sigma, 0.f)));
                ok = (sigma >= 0.f) && (alpha >= kAlphaMin);
                z = a.w;
            }
            const u64 okm = __ballot(ok);
            // T through the batch in list order; lane j keeps entry j's weight
            float wv = 0.f;
            u64 valid = 0ull;
            for (u32 j = 0; j < bn; ++j) {
                if (!((okm >> j) & 1ull))
                    continue;
                const float al = lane_f(alpha, (int)j);
                const float next_T = uniform_f(T * (1.0f - al));
                if (next_T <= kTMin) { // terminates: not counted, nothing behind it either
                    done = true;
                    break;
                }
                const float w = uniform_f(al * T);
                wv = (u32)lane == j ? w : wv;
                valid |= 1ull << j;
                T = next_T;
            }
            // front to back, lanes = channels
            const int n_valid = __popcll(valid);
            for (int i = 0; i < n_valid; ++i) {
                const int j = __ffsll((long long)valid) - 1;
                valid &= valid - 1ull;
                const float w = lane_f(wv, j);
                const u32 g = (u32)__builtin_amdgcn_readlane((int)gid, j);
                const float4 x = load4<VEC>(X + (int64_t)g * ldx, c, D);
                acc.x = __builtin_fmaf(w, x.x, acc.x);
                acc.y = __builtin_fmaf(w, x.y, acc.y);
                acc.z = __builtin_fmaf(w, x.z, acc.z);
                acc.w = __builtin_fmaf(w, x.w, acc.w);
                zacc = __builtin_fmaf(w, lane_f(z, j), zacc);
            }
        }
    }
    store4<false>(out + (int64_t)probe * D, c, D, acc);
    if (chunk == 0 && lane == 0) {
        if (depth)
            depth[probe] = zacc;
        if (alpha_out)
            alpha_out[probe] = 1.0f - T;
    }
}

bool rows_vec(const float *X, int64_t ldx) { return !(reinterpret_cast<uintptr_t>(X) & 15) && !(ldx & 3); }

} // namespace

int launch_prompt_scores(int64_t N, int D, int P, int n_pos, const void *X, int mt, int64_t ldx, const float *prompts, int normalize,
                         const float *threshold, uint8_t *mask, float *scores, hipStream_t s)
{
    if (N == 0)
        return GWBP_OK;
    unsigned grid;
    if (int rc = grid_of("prompt_scores", N, &grid, kQRows))
        return rc;
    const int use_thr = threshold ? 1 : 0;
    const float thr = threshold ? *threshold : 0.f;
    if (mt != GWBP_MAP_F32) // the half instantiations are query_half.hip's
        launch_prompt_scores_half(grid, s, N, D, P, n_pos, X, mt, ldx, prompts, normalize, use_thr, thr, mask, scores);
    else
        launch_prompt_scores_t<GWBP_MAP_F32>(grid, s, N, D, P, n_pos, X, ldx, prompts, normalize, use_thr, thr, mask, scores);
    return check_hip(hipGetLastError(), "prompt_scores launch");
}

int launch_probe_pixels(const Ws &W, const ViewDev &V, int M, const int32_t *xy, const float *X, int64_t ldx, int D, float *out,
                        float *depth, float *alpha, hipStream_t s)
{
    const int n_tiles = V.tile_w * V.tile_h;
    const int fin = sort_passes(n_tiles) & 1;
    const dim3 grid((unsigned)M, (unsigned)((D + kProbeChunk - 1) / kProbeChunk));
    if (rows_vec(X, ldx))
        hipLaunchKernelGGL(k_probe_pixels<true>, grid, dim3(64), 0, s, V, W.tile_offsets, W.vals[fin], W.g2d, xy, X, ldx, D, out, depth,
                           alpha);
    else
        hipLaunchKernelGGL(k_probe_pixels<false>, grid, dim3(64), 0, s, V, W.tile_offsets, W.vals[fin], W.g2d, xy, X, ldx, D, out, depth,
                           alpha);
    return check_hip(hipGetLastError(), "probe_pixels launch");
}

} // namespace gwbp
