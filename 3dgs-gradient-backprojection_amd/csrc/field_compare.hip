// field_compare.hip -- gwbp_field_compare's launcher, the fp32-field instantiations of k_field_compare (field_compare_kernel.h: the
// kernel and its contract) and k_compare_table, the per-view sums of the rows' partial sums.
#include "gwbp_dev.h"
#include "field_compare_kernel.h"

namespace gwbp {

namespace {

constexpr int kTableThreads = 1024;

// table[0..5] = the rows' sums in a fixed order; table[6] = H W, table[7] = D.  One workgroup.
__global__ __launch_bounds__(kTableThreads) void k_compare_table(ViewDev V, int D, const double *__restrict__ rowsums,
                                                                 double *__restrict__ table)
{
    __shared__ double s[kRowSums][kTableThreads];
    const int tid = threadIdx.x;
    const int n_rows = V.tile_w * V.tile_h * 16;
    double a[kRowSums];
#pragma unroll
    for (int k = 0; k < kRowSums; ++k)
        a[k] = 0.0;
    for (int r0 = 0; r0 < n_rows; r0 += kTableThreads) { // uniform trip count; the rows below the image were never written
        const int r = r0 + tid;
        const int iy = ((r >> 4) / V.tile_w) * kTile + (r & 15);
        if (r < n_rows && iy < V.H) {
#pragma unroll
            for (int k = 0; k < kRowSums; ++k)
                a[k] += rowsums[(size_t)r * kRowSums + k];
        }
    }
#pragma unroll
    for (int k = 0; k < kRowSums; ++k)
        s[k][tid] = a[k];
    __syncthreads();
    for (int half = kTableThreads / 2; half > 0; half >>= 1) {
        if (tid < half) {
#pragma unroll
            for (int k = 0; k < kRowSums; ++k)
                s[k][tid] += s[k][tid + half];
        }
        __syncthreads();
    }
    if (tid < kRowSums)
        table[tid] = s[tid][0];
    if (tid == kRowSums)
        table[6] = (double)V.H * (double)V.W;
    if (tid == kRowSums + 1)
        table[7] = (double)D;
}

} // namespace

size_t field_compare_scratch_bytes(int n_tiles) { return (size_t)n_tiles * 16u * kRowSums * sizeof(double); }

int launch_field_compare(const Layout &L, const Ws &W, const ViewDev &V, const void *feats, int ft, int64_t ldf, int D, const void *map,
                         int mt, int64_t ms_y, int64_t ms_x, int lr_h, int lr_w, const int32_t *ymap, const int32_t *xmap,
                         float *planes, double *table, hipStream_t s)
{
    const int n_tiles = V.tile_w * V.tile_h;
    const unsigned grid = (unsigned)((n_tiles + 7) & ~7) * 4u;
    // the rows' sums live in the carry slices of the 256-channel scatter kernel, which nothing reads between two scatters
    double *rowsums = reinterpret_cast<double *>(W.carry);
    const CmpMap M{map, ms_y, ms_x, ymap, xmap, lr_h, lr_w};
    // four-element loads of the field and of the map (16 B of fp32, 8 B of halves) where every row of both allows them; same bits
    // either way
    const uintptr_t malign = mt == GWBP_MAP_F32 ? 15 : 7;
    const bool vec = D % 4 == 0 && field_rows_vec(feats, ldf, ft) &&
                     (reinterpret_cast<uintptr_t>(map) & malign) == 0 && ms_y % 4 == 0 && ms_x % 4 == 0;
    const bool wide2 = vec && D >= 512;
    const int empty = L.n == 0;
    if (ft != GWBP_MAP_F32) // the half-field instantiations are field_compare_half.hip's
        launch_field_compare_half(ft, mt, wide2, vec, grid, s, V, empty, W, feats, ldf, D, &M, planes, rowsums);
    else
        launch_compare_ft<GWBP_MAP_F32>(mt, wide2, vec, grid, s, V, empty, W, feats, ldf, D, M, planes, rowsums);
    int rc = check_hip(hipGetLastError(), "field_compare launch");
    if (rc)
        return rc;
    hipLaunchKernelGGL(k_compare_table, dim3(1), dim3(kTableThreads), 0, s, V, D, rowsums, table);
    return check_hip(hipGetLastError(), "field_compare table launch");
}

} // namespace gwbp
