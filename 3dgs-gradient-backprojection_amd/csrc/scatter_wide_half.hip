// scatter_wide_half.hip -- k_scatter_wide over fp16 / bf16 maps (gwbp_scatter_typed and its upsampled / bilinear forms): the
// kernel of scatter_wide.hip, whose fp32 instantiations stay alone in their object (tests/test_capi_cpu.py pins their code),
// instantiated for the two half types.  The slab is staged with 2-B loads that land as raw bits in the same 32 landing registers
// and are widened when the slab is written into LDS; everything behind the slab is the fp32 kernel's.  The Makefile runs the
// same assembly gate over this object (tools/check_asm_hazards.py --wide --kernels 4).
#include "gwbp_dev.h"

#undef GWBP_STAMPS // the in-kernel stamps (PROFILE builds) are the fp32 kernel's only

#include "scatter_wide_kernel.h"

namespace gwbp {

int launch_scatter_wide_half(const Layout &L, const Ws &W, const ViewDev &V, const FeatMap &M, int D, float scale_f, float *F,
                             hipStream_t s, int mt)
{
    if (mt == GWBP_MAP_F16)
        return launch_scatter_wide_t<GWBP_MAP_F16>(L, W, V, M, D, scale_f, F, s);
    if (mt == GWBP_MAP_BF16)
        return launch_scatter_wide_t<GWBP_MAP_BF16>(L, W, V, M, D, scale_f, F, s);
    return set_error(GWBP_EINVAL, "scatter_wide: unknown map type %d", mt);
}

} // namespace gwbp
