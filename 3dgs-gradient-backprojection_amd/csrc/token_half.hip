// token_half.hip -- k_token_apply over fp16 / bf16 token maps (gwbp_scatter_tokens_typed): the kernel of token.hip, whose fp32
// instantiations stay alone in their object, instantiated for the two half types.  Token rows are widened to fp32 as they are
// read (8-B loads of four channels); the sums and their order are the fp32 kernel's, so F and d equal it bit for bit.
#include "token_kernel.h"

namespace gwbp {

int launch_token_apply_half(const Layout &L, const Ws &W, const ViewDev &V, const void *tokens, int64_t ts_y, int64_t ts_x,
                            int D, const int32_t *ymap, const int32_t *xmap, float scale_f, float scale_d, float *F, float *d,
                            hipStream_t s, int mt)
{
    if (mt == GWBP_MAP_F16)
        return launch_token_apply_t<GWBP_MAP_F16>(L, W, V, tokens, ts_y, ts_x, D, ymap, xmap, scale_f, scale_d, F, d, s);
    if (mt == GWBP_MAP_BF16)
        return launch_token_apply_t<GWBP_MAP_BF16>(L, W, V, tokens, ts_y, ts_x, D, ymap, xmap, scale_f, scale_d, F, d, s);
    return set_error(GWBP_EINVAL, "token_apply: unknown map type %d", mt);
}

} // namespace gwbp
