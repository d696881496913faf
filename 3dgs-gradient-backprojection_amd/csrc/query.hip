// query.hip -- questions asked of a finished [N, D] feature field (the reference's segment.py / segment_compressed.py /
// click_and_segment.py: get_mask3d_lseg, and the render of the field that the click script reads one pixel of):
//
//   k_prompt_scores   s[g, j] = X[g] . prompts[j] (/ max(|X[g]|, 1e-12)),  j < P <= 32, and the 3-D mask
//                     max_{j < n_pos} s[g, j] > max_{j >= n_pos} s[g, j]  (&& s[g, 0] > threshold): ONE pass over X
//   k_probe_pixels    out[m, :] = sum_g w_g(p_m) X[g, :] at M pixels only, + the accumulated depth and alpha of those pixels
//
// Both kernels are query_kernel.h's, templates over the element type of X: this file instantiates them for fp32 fields,
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

int launch_probe_pixels(const Ws &W, const ViewDev &V, int M, const int32_t *xy, const void *X, int mt, int64_t ldx, int D, float *out,
                        float *depth, float *alpha, hipStream_t s)
{
    if (mt != GWBP_MAP_F32) // the half instantiations are query_half.hip's
        launch_probe_pixels_half(W, V, M, xy, X, mt, ldx, D, out, depth, alpha, s);
    else
        launch_probe_pixels_t<GWBP_MAP_F32>(W, V, M, xy, X, ldx, D, out, depth, alpha, s);
    return check_hip(hipGetLastError(), "probe_pixels launch");
}

} // namespace gwbp
