// query_half.hip -- the fp16 / bf16 instantiations of k_prompt_scores and k_probe_pixels (query_kernel.h): a half field is widened as it is loaded, so the
// staged values, the chains and every result are those of the fp32 kernel on the widened field.
#include "gwbp_dev.h"
#include "query_kernel.h"

namespace gwbp {

void launch_prompt_scores_half(unsigned grid, hipStream_t s, int64_t N, int D, int P, int n_pos, const void *X, int mt, int64_t ldx,
                               const float *prompts, int normalize, int use_thr, float thr, uint8_t *mask, float *scores)
{
    if (mt == GWBP_MAP_F16)
        launch_prompt_scores_t<GWBP_MAP_F16>(grid, s, N, D, P, n_pos, X, ldx, prompts, normalize, use_thr, thr, mask, scores);
    else
        launch_prompt_scores_t<GWBP_MAP_BF16>(grid, s, N, D, P, n_pos, X, ldx, prompts, normalize, use_thr, thr, mask, scores);
}

void launch_probe_pixels_half(const Ws &W, const ViewDev &V, int M, const int32_t *xy, const void *X, int mt, int64_t ldx, int D,
                              float *out, float *depth, float *alpha, hipStream_t s)
{
    if (mt == GWBP_MAP_F16)
        launch_probe_pixels_t<GWBP_MAP_F16>(W, V, M, xy, X, ldx, D, out, depth, alpha, s);
    else
        launch_probe_pixels_t<GWBP_MAP_BF16>(W, V, M, xy, X, ldx, D, out, depth, alpha, s);
}

} // namespace gwbp
