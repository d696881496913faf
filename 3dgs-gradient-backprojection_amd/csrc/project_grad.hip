// project_grad.hip -- backward of the projection (k_project) for one view: from v_g2d [N, 6], the gradient of each projected record
// that the blend backward leaves (render_grad.hip), to the gradients of means / quats / scales / opacities and of the view matrix.
//
// One lane per Gaussian, k_project's block size and its coalesced AoS loads (12 / 16 / 12 / 4 B per lane + the 24-B v_g2d row + the
// record's radius), 44 B written per lane.  The per-Gaussian product is project_grad.h's project_vjp in float64, which recomputes the
// forward from the stored float32 inputs; each output is that double rounded once, WRITTEN (not added).  A row the projection culled
// (radius 0 in the workspace's record) stores zeros and is never evaluated.
//
// The view-matrix gradient is a sum over all visible rows of 12 doubles, taken without atomics and in a fixed order: the lanes of a
// wave by shuffles, the waves of a block in LDS in wave order, each block's 12 partial sums with plain stores into the caller's
// scratch [n_blocks, 12], and a second one-workgroup kernel over the blocks in block order.  Same inputs, same bits.
#include "gwbp_dev.h"
#include "project_grad.h"

namespace gwbp {

constexpr int kViewGrad = 12; // d / d(R[9] row-major, t[3])

template <int CAM, bool AA>
__global__ __launch_bounds__(kScanBlock) void k_project_bwd(
    int64_t N, ViewDev V, const float *__restrict__ means, const float *__restrict__ quats, const float *__restrict__ scales,
    const float *__restrict__ opac, const G2D *__restrict__ g2d, const float *__restrict__ v_g2d, float *__restrict__ v_means,
    float *__restrict__ v_quats, float *__restrict__ v_scales, float *__restrict__ v_opac, double *__restrict__ partials)
{
    const int64_t i = (int64_t)blockIdx.x * kScanBlock + threadIdx.x;
    ProjGrad g;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        g.mean[k] = g.scale[k] = g.t[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        g.quat[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k)
        g.R[k] = 0.0;
    g.opacity = 0.0;

    const bool visible = i < N && g2d[i].radius > 0;
    if (visible) { // (a culled row is never evaluated: nothing non-finite can come from it)
        ProjViewF P;
#pragma unroll
        for (int k = 0; k < 9; ++k)
            P.R[k] = V.R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            P.t[k] = V.t[k];
        P.fx = V.fx, P.fy = V.fy, P.cx = V.cx, P.cy = V.cy, P.W = V.W, P.H = V.H, P.eps2d = V.eps2d;
        const float m[3] = {means[3 * i], means[3 * i + 1], means[3 * i + 2]};
        const float4 q4 = reinterpret_cast<const float4 *>(quats)[i];
        const float q[4] = {q4.x, q4.y, q4.z, q4.w};
        const float s[3] = {scales[3 * i], scales[3 * i + 1], scales[3 * i + 2]};
        float v[6];
#pragma unroll
        for (int k = 0; k < 6; ++k)
            v[k] = v_g2d[6 * i + k];
        project_vjp_stored<CAM, AA>(P, m, q, s, opac[i], v, g);
    }
    if (i < N) {
        if (v_means)
            v_means[3 * i] = (float)g.mean[0], v_means[3 * i + 1] = (float)g.mean[1], v_means[3 * i + 2] = (float)g.mean[2];
        if (v_quats)
            reinterpret_cast<float4 *>(v_quats)[i] = make_float4((float)g.quat[0], (float)g.quat[1], (float)g.quat[2], (float)g.quat[3]);
        if (v_scales)
            v_scales[3 * i] = (float)g.scale[0], v_scales[3 * i + 1] = (float)g.scale[1], v_scales[3 * i + 2] = (float)g.scale[2];
        if (v_opac)
            v_opac[i] = (float)g.opacity;
    }

    // The view sums.  `partials` is a kernel argument: the branch is uniform over the grid, and inside it every thread of the block --
    // out of range and hidden lanes with zeros -- takes part in every shuffle and reaches the one barrier.
    if (partials) {
        __shared__ double s_wave[kScanBlock / 64][kViewGrad];
        double acc[kViewGrad];
#pragma unroll
        for (int k = 0; k < 9; ++k)
            acc[k] = g.R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            acc[9 + k] = g.t[k];
#pragma unroll
        for (int k = 0; k < kViewGrad; ++k)
#pragma unroll
            for (int o = 32; o > 0; o >>= 1)
                acc[k] += __shfl_down(acc[k], o, 64);
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < kViewGrad; ++k)
                s_wave[wave][k] = acc[k];
        }
        __syncthreads();
        if (threadIdx.x < kViewGrad) {
            double sum = s_wave[0][threadIdx.x];
#pragma unroll
            for (int w = 1; w < kScanBlock / 64; ++w)
                sum += s_wave[w][threadIdx.x];
            partials[(int64_t)blockIdx.x * kViewGrad + threadIdx.x] = sum;
        }
    }
}

// The blocks' partial sums in block order: thread (c, k) adds value k of the blocks of chunk c, first to last; after the barrier the
// chunks are added first to last.  One workgroup; every thread reaches the barrier.
constexpr int kSumChunks = 21; // 21 x 12 = 252 of 256 threads
__global__ __launch_bounds__(256) void k_project_bwd_sum(int n_blocks, const double *__restrict__ partials, double *__restrict__ out)
{
    __shared__ double s_chunk[kSumChunks][kViewGrad];
    const int c = threadIdx.x / kViewGrad, k = threadIdx.x % kViewGrad;
    const int per = (n_blocks + kSumChunks - 1) / kSumChunks;
    if (c < kSumChunks) {
        double sum = 0.0;
        const int end = min(n_blocks, (c + 1) * per);
        for (int b = c * per; b < end; ++b)
            sum += partials[(int64_t)b * kViewGrad + k];
        s_chunk[c][k] = sum;
    }
    __syncthreads();
    if (threadIdx.x < kViewGrad) {
        double sum = s_chunk[0][threadIdx.x];
        for (int j = 1; j < kSumChunks; ++j)
            sum += s_chunk[j][threadIdx.x];
        out[threadIdx.x] = sum;
    }
}

int project_backward_blocks(int64_t n) { return (int)((n + kScanBlock - 1) / kScanBlock); }

int launch_project_bwd(const Layout &L, const Ws &W, const ViewDev &V, int camera_model, int rasterize_mode, const float *means,
                       const float *quats, const float *scales, const float *opac, const float *v_g2d, float *v_means, float *v_quats,
                       float *v_scales, float *v_opac, double *v_viewmat, double *scratch, hipStream_t s)
{
    if (L.n == 0) {
        if (v_viewmat)
            return check_hip(hipMemsetAsync(v_viewmat, 0, kViewGrad * sizeof(double), s), "memset v_viewmat");
        return GWBP_OK;
    }
    const bool aa = rasterize_mode == GWBP_RASTERIZE_ANTIALIASED;
    decltype(&k_project_bwd<kGradPinhole, false>) k = nullptr;
    switch (camera_model) {
    case GWBP_CAMERA_PINHOLE: k = aa ? k_project_bwd<kGradPinhole, true> : k_project_bwd<kGradPinhole, false>; break;
    case GWBP_CAMERA_ORTHO: k = aa ? k_project_bwd<kGradOrtho, true> : k_project_bwd<kGradOrtho, false>; break;
    case GWBP_CAMERA_FISHEYE: k = aa ? k_project_bwd<kGradFisheye, true> : k_project_bwd<kGradFisheye, false>; break;
    default: return set_error(GWBP_EINVAL, "unknown camera model %d", camera_model);
    }
    hipLaunchKernelGGL(k, dim3(L.n_scan_blocks), dim3(kScanBlock), 0, s, L.n, V, means, quats, scales, opac, W.g2d, v_g2d, v_means,
                       v_quats, v_scales, v_opac, v_viewmat ? scratch : nullptr);
    if (v_viewmat)
        hipLaunchKernelGGL(k_project_bwd_sum, dim3(1), dim3(256), 0, s, L.n_scan_blocks, scratch, v_viewmat);
    return check_hip(hipGetLastError(), "project_bwd launch");
}

} // namespace gwbp
