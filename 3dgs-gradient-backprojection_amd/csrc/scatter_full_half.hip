// scatter_full_half.hip -- k_scatter_full over fp16 / bf16 maps: the kernel of scatter_full.hip (whose fp32 instantiations stay
// alone in their object) instantiated for the two half types, with the channel-contiguous staging forms only -- VEC 1 (full
// resolution, and the nearest-index form of gwbp_scatter_upsampled_typed) and VEC 2 (bilinear).  A unit of the staging is still
// four channels of one pixel: one 8-B load instead of 16 B, widened where it is written into the fp32 slab.
#include "scatter_full_kernel.h"

namespace gwbp {

namespace {

template <int MT>
int launch_half(const Layout &L, const Ws &W, const ViewDev &V, const FeatMap &M, int D, float scale_f, float scale_d, float *F,
                float *d, hipStream_t s)
{
    const bool bil = M.bilinear();
    const void *fn = bil ? reinterpret_cast<const void *>(k_scatter_full<false, 2, MT>)
                         : reinterpret_cast<const void *>(k_scatter_full<false, 1, MT>);
    int rc = ensure_dynamic_lds(fn, (int)kLdsBytes);
    if (rc)
        return rc;
    int n_cu = 0;
    if ((rc = device_cus(&n_cu)))
        return rc;
    // the fp32 launch's grid: one persistent workgroup per CU (caps.scatter_workgroups overrides), a multiple of 8
    int grid = L.scatter_wgs > 0 ? L.scatter_wgs : n_cu;
    grid = (grid + 7) & ~7;
    u32 *queues = W.shards + kShards * 16;
    const int dbg = profile_knob("GWBP_ABLATE");
    if (bil)
        hipLaunchKernelGGL((k_scatter_full<false, 2, MT>), dim3(grid), dim3(kThreads), kLdsBytes, s, V, D / kChunk,
                           W.tile_offsets, W.hdr_count, W.headers, W.wpool, M, kChunk, D, scale_f, scale_d, F, d, queues, dbg);
    else
        hipLaunchKernelGGL((k_scatter_full<false, 1, MT>), dim3(grid), dim3(kThreads), kLdsBytes, s, V, D / kChunk,
                           W.tile_offsets, W.hdr_count, W.headers, W.wpool, M, kChunk, D, scale_f, scale_d, F, d, queues, dbg);
    return check_hip(hipGetLastError(), "scatter_full launch");
}

} // namespace

int launch_scatter_full_half(const Layout &L, const Ws &W, const ViewDev &V, const FeatMap &M, int D, float scale_f,
                             float scale_d, float *F, float *d, hipStream_t s, int mt)
{
    // 8-B staging loads of four channels: channel-contiguous pixels whose rows start on 16 B (strides in elements)
    const bool aligned = M.fs_c == 1 && (M.fs_x % 8 == 0) && (M.fs_y % 8 == 0) && ((reinterpret_cast<uintptr_t>(M.p) & 15) == 0);
    if (D % kChunk != 0 || !aligned || M.enc)
        return set_error(GWBP_EUNSUPPORTED, "half-precision map: the 128-channel kernel needs D %% 128 == 0, fs_c == 1, fs_x and fs_y "
                                            "multiples of 8 elements and a 16-B aligned map (D=%d strides %lld %lld %lld)",
                         D, (long long)M.fs_y, (long long)M.fs_x, (long long)M.fs_c);
    if (mt == GWBP_MAP_F16)
        return launch_half<GWBP_MAP_F16>(L, W, V, M, D, scale_f, scale_d, F, d, s);
    if (mt == GWBP_MAP_BF16)
        return launch_half<GWBP_MAP_BF16>(L, W, V, M, D, scale_f, scale_d, F, d, s);
    return set_error(GWBP_EINVAL, "scatter_full: unknown map type %d", mt);
}

} // namespace gwbp
