// render_wide_half.hip -- the instantiations of k_render_rows / k_render_rows4 (render_wide_kernel.h) with a half colour table, a half
// output or both: the table's bits are widened in process(), the output is narrowed in the store epilogue, and everything between is the
// fp32 kernel's.
#include "gwbp_dev.h"
#include "render_wide_kernel.h"

namespace gwbp {

void launch_render_half(const Ws &W, const ViewDev &V, const void *colors, int mt, int64_t ldc, int D, void *out, int ot, hipStream_t s)
{
    with_map_type(mt, [&](auto MT) {
        with_map_type(ot, [&](auto OT) {
            if constexpr (MT != GWBP_MAP_F32 || OT != GWBP_MAP_F32) // (that pair is render_wide.hip's)
                launch_render_t<MT, OT>(W, V, colors, ldc, D, out, s);
        });
    });
}

} // namespace gwbp
