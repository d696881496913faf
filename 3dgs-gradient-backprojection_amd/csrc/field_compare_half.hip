// field_compare_half.hip -- the instantiations of k_field_compare (field_compare_kernel.h) for fp16 / bf16 FIELDS, each against every
// map type: the field's bits are widened in the walk's process() step, everything behind it is the fp32 kernel's.
#include "gwbp_dev.h"
#include "field_compare_kernel.h"

namespace gwbp {

void launch_field_compare_half(int ft, int mt, bool wide2, bool vec, unsigned grid, hipStream_t s, const ViewDev &V, int empty, const Ws &W,
                               const void *feats, int64_t ldf, int D, const void *cmp_map, float *planes, double *rowsums)
{
    const CmpMap &M = *static_cast<const CmpMap *>(cmp_map);
    if (ft == GWBP_MAP_F16)
        launch_compare_ft<GWBP_MAP_F16>(mt, wide2, vec, grid, s, V, empty, W, feats, ldf, D, M, planes, rowsums);
    else
        launch_compare_ft<GWBP_MAP_BF16>(mt, wide2, vec, grid, s, V, empty, W, feats, ldf, D, M, planes, rowsums);
}

} // namespace gwbp
