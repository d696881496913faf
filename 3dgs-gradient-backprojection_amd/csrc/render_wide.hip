// render_wide.hip -- gwbp_render's launcher and the fp32 instantiations of k_render_rows / k_render_rows4 (render_wide_kernel.h: the
// kernels and their contract); a half colour table or a half output takes render_wide_half.hip's.
#include "gwbp_dev.h"
#include "render_wide_kernel.h"

namespace gwbp {

int launch_render(const Layout &L, const Ws &W, const ViewDev &V, const void *colors, int mt, int64_t ldc, int D, void *out, int ot,
                  hipStream_t s)
{
    (void)L;
    if (mt != GWBP_MAP_F32 || ot != GWBP_MAP_F32)
        launch_render_half(W, V, colors, mt, ldc, D, out, ot, s);
    else
        launch_render_t<GWBP_MAP_F32, GWBP_MAP_F32>(W, V, colors, ldc, D, out, s);
    return check_hip(hipGetLastError(), "render launch");
}

} // namespace gwbp
