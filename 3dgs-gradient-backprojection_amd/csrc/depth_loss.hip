// depth_loss.hip -- the depth supervision of training: the loss of a render's expected depth against the view's
// triangulated points (the reference trainer's depth_loss) or against a depth map, and its gradient with respect to the render and
// the alpha map.  depth_math.h carries every expression that is not a memory access.
//
//   k_depth_points_fwd   a thread per point: the four corners of the accumulated depth A are read IN PLACE (element stride Dp, channel
//                        ch of the [H, W, Dp] render; no copy of the channel) with the alpha map beside them, a corner outside the
//                        image is +0 and issues no load.  The workgroup's sum of t in float64 goes to the workspace.
//   k_depth_points_bwd   a thread per point: the sample is recomputed from A and a (nothing per point was saved), multiplied by the
//                        upstream gradient READ FROM THE DEVICE, and its four shares are added into channel ch of a zero-filled
//                        [H, W, Dp] gradient and a zero-filled [H, W] alpha gradient with float atomics.  A corner outside the image
//                        and a share that is zero issue nothing.  Points share corners: the order of those adds is not fixed, the
//                        output is not bit-reproducible.
//   k_depth_map_fwd      a thread per kMapPer pixels, consecutive lanes on consecutive pixels; VEC4 (Dp == 4, a 16-B aligned render):
//                        the pixel's four channels in one 16-B load.  The workgroup's sums of w t and w in float64 go to the workspace.
//   k_depth_map_bwd      the same walk; every pixel's Dp render gradients (zeros but for channel ch; VEC4: one 16-B store) and its
//                        alpha gradient are STORED: no atomics, no zero-fill, the same bits every run.
//   k_depth_finish       one workgroup: the partials in ascending index order (they pass through LDS), then the float32 loss and,
//                        for the map term, the two float64 sums the backward reads.
//
// The reduction has a fixed shape: wave_sum_d (gwbp_dev.h: the DPP steps of wave_sum on a double), the four waves in wave
// order, the workgroups in index order.  The loss is a function of the inputs alone.  Nothing is read back to the host.
// Every index is guarded: a point's corner is used only when 0 <= row < H and 0 <= column < W (float comparisons before any
// conversion, so NaN and huge coordinates touch nothing), a pixel only below H W; loop bounds are kernel arguments.
#include "gwbp_dev.h"
#include "depth_math.h"

namespace gwbp {

namespace {

constexpr int kBlock = GWBP_DEPTH_BLOCK; // points per workgroup
constexpr int kMapPer = 4;               // pixels per thread of the map kernels
constexpr int kFinishChunk = 1024;       // workgroups whose partials pass through LDS at once
static_assert(kBlock == 256, "the reductions below are written for four waves");

struct DepthImage { // wave-uniform
    int H, W, Dp, ch;
    const float *render; // [H, W, Dp]
    const float *alpha;  // [H, W]
};

struct Corner {
    bool in;
    int64_t pix;
    float A, a, e;
};

// the pixel (yf, xf) -- floats that hold integers, or anything else for a point that lies nowhere
__device__ __forceinline__ Corner fetch_corner(const DepthImage &I, float yf, float xf)
{
    Corner c;
    c.in = yf >= 0.0f && yf < (float)I.H && xf >= 0.0f && xf < (float)I.W; // (H, W <= 2^24: exact)
    c.pix = 0, c.A = 0.0f, c.a = 0.0f, c.e = 0.0f;
    if (c.in) {
        c.pix = (int64_t)(int)yf * I.W + (int)xf;
        c.A = I.render[c.pix * I.Dp + I.ch];
        c.a = I.alpha[c.pix];
        c.e = depth_expected(c.A, c.a);
    }
    return c;
}

__device__ __forceinline__ DepthSample sample_point(const DepthImage &I, float x, float y, float g, Corner c[4])
{
    const float x0 = floorf(x), y0 = floorf(y);
    c[0] = fetch_corner(I, y0, x0);
    c[1] = fetch_corner(I, y0, x0 + 1.0f);
    c[2] = fetch_corner(I, y0 + 1.0f, x0);
    c[3] = fetch_corner(I, y0 + 1.0f, x0 + 1.0f);
    return depth_sample(x, y, x0, y0, c[0].e, c[1].e, c[2].e, c[3].e, g);
}

// the workgroup's sums of K per-thread float64 terms, to partial[block * K + k]
template <int K>
__device__ __forceinline__ void block_sums(double (&v)[K], double *__restrict__ partial, int64_t block)
{
    __shared__ double red[4][K];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double s = wave_sum_d(v[k]); // (every lane of the workgroup is here: the callers return nowhere before)
        if (lane == 0)
            red[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < K)
        partial[block * K + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

__global__ __launch_bounds__(kBlock) void k_depth_points_fwd(DepthImage I, int M, const float *__restrict__ points,
                                                             const float *__restrict__ depths, float *__restrict__ per_point,
                                                             double *__restrict__ partial)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double v[2] = {0.0, 0.0};
    if (i < M) {
        Corner c[4];
        const DepthSample S = sample_point(I, points[2 * i], points[2 * i + 1], depths[i], c);
        v[0] = (double)S.t, v[1] = 1.0;
        if (per_point)
            per_point[2 * i] = S.d, per_point[2 * i + 1] = S.t;
    }
    block_sums<2>(v, partial, blockIdx.x);
}

__global__ __launch_bounds__(kBlock) void k_depth_points_bwd(DepthImage I, int M, const float *__restrict__ points,
                                                             const float *__restrict__ depths, const float *__restrict__ upstream,
                                                             float scale_over_m, float *__restrict__ v_render,
                                                             float *__restrict__ v_alpha)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= M)
        return;
    Corner c[4];
    const DepthSample S = sample_point(I, points[2 * i], points[2 * i + 1], depths[i], c);
    float v_e[4];
    depth_corner_shares(S, depth_sample_grad(S, upstream[0] * scale_over_m), v_e);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!c[k].in)
            continue;
        float v_A, v_a;
        depth_expected_grad(c[k].A, c[k].a, v_e[k], v_A, v_a);
        if (v_A != 0.0f)
            atomicAdd(v_render + c[k].pix * I.Dp + I.ch, v_A);
        if (v_a != 0.0f)
            atomicAdd(v_alpha + c[k].pix, v_a);
    }
}

struct DepthMap { // wave-uniform
    const float *g; // [H, W]
    const float *w; // [H, W] or nullptr
    int kind;
};

template <bool VEC4>
__device__ __forceinline__ float load_depth(const DepthImage &I, int64_t p)
{
    if (VEC4) {
        const float4 r = *reinterpret_cast<const float4 *>(I.render + 4 * p);
        return I.ch == 0 ? r.x : I.ch == 1 ? r.y : I.ch == 2 ? r.z : r.w;
    }
    return I.render[p * I.Dp + I.ch];
}

template <bool VEC4>
__global__ __launch_bounds__(kBlock) void k_depth_map_fwd(DepthImage I, DepthMap T, int64_t pixels, double *__restrict__ partial)
{
    double v[2] = {0.0, 0.0};
#pragma unroll
    for (int j = 0; j < kMapPer; ++j) {
        const int64_t p = ((int64_t)blockIdx.x * kMapPer + j) * kBlock + threadIdx.x;
        if (p >= pixels)
            continue;
        const float g = T.g[p], w = T.w ? T.w[p] : 1.0f;
        if (g > 0.0f && w > 0.0f) {
            const float e = depth_expected(load_depth<VEC4>(I, p), I.alpha[p]);
            v[0] += (double)w * (double)fabsf(depth_map_residual(T.kind, e, g));
            v[1] += (double)w;
        }
    }
    block_sums<2>(v, partial, blockIdx.x);
}

template <bool VEC4>
__global__ __launch_bounds__(kBlock) void k_depth_map_bwd(DepthImage I, DepthMap T, int64_t pixels, const double *__restrict__ sums,
                                                          const float *__restrict__ upstream, float scale,
                                                          float *__restrict__ v_render, float *__restrict__ v_alpha)
{
    const double sw = sums[1];
    const float c = sw > 0.0 ? (float)((double)upstream[0] * (double)scale / sw) : 0.0f; // float64, rounded once
#pragma unroll
    for (int j = 0; j < kMapPer; ++j) {
        const int64_t p = ((int64_t)blockIdx.x * kMapPer + j) * kBlock + threadIdx.x;
        if (p >= pixels)
            continue;
        const float g = T.g[p], w = T.w ? T.w[p] : 1.0f;
        float v_A = 0.0f, v_a = 0.0f;
        if (g > 0.0f && w > 0.0f) {
            const float A = load_depth<VEC4>(I, p), a = I.alpha[p];
            depth_expected_grad(A, a, depth_map_grad(T.kind, depth_expected(A, a), g, w * c), v_A, v_a);
        }
        if (VEC4) {
            *reinterpret_cast<float4 *>(v_render + 4 * p) =
                make_float4(I.ch == 0 ? v_A : 0.0f, I.ch == 1 ? v_A : 0.0f, I.ch == 2 ? v_A : 0.0f, I.ch == 3 ? v_A : 0.0f);
        } else {
            for (int k = 0; k < I.Dp; ++k)
                v_render[p * I.Dp + k] = k == I.ch ? v_A : 0.0f;
        }
        v_alpha[p] = v_a;
    }
}

// loss = scale (sum of partial[2 b]) / (sum of partial[2 b + 1]) over the n workgroups b in ascending order, 0 where the second sum is
// not positive; sums (or nullptr) takes the two float64 sums
__global__ __launch_bounds__(kBlock) void k_depth_finish(int64_t n, const double *__restrict__ partial, float scale,
                                                         float *__restrict__ loss, double *__restrict__ sums)
{
    __shared__ double buf[kFinishChunk * 2];
    __shared__ double total[2];
    double s = 0.0;
    for (int64_t b0 = 0; b0 < n; b0 += kFinishChunk) {
        const int m = (int)min((int64_t)kFinishChunk, n - b0) * 2;
        __syncthreads();
        for (int i = threadIdx.x; i < m; i += kBlock)
            buf[i] = partial[b0 * 2 + i];
        __syncthreads();
        if (threadIdx.x < 2)
            for (int i = (int)threadIdx.x; i < m; i += 2)
                s += buf[i];
    }
    if (threadIdx.x < 2)
        total[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        loss[0] = total[1] > 0.0 ? (float)((double)scale * total[0] / total[1]) : 0.0f;
        if (sums)
            sums[0] = total[0], sums[1] = total[1];
    }
}

int64_t map_blocks(int64_t pixels) { return (pixels + (int64_t)kMapPer * kBlock - 1) / ((int64_t)kMapPer * kBlock); }

DepthImage image_of(int H, int W, int Dp, int ch, const float *render, const float *alpha)
{
    DepthImage I;
    I.H = H, I.W = W, I.Dp = Dp, I.ch = ch, I.render = render, I.alpha = alpha;
    return I;
}

bool vec4_layout(int Dp, const void *a, const void *b) { return Dp == 4 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0; }

} // namespace

size_t depth_points_workspace_bytes(int64_t M) { return (size_t)((M + kBlock - 1) / kBlock) * 2 * sizeof(double); }
size_t depth_map_workspace_bytes(int H, int W) { return (size_t)map_blocks((int64_t)H * W) * 2 * sizeof(double); }

int launch_depth_points_loss(int H, int W, int Dp, int ch, const float *render, const float *alpha, int64_t M, const float *points,
                             const float *depths, float scale, float *loss, float *per_point, double *ws, hipStream_t s)
{
    const int64_t blocks = (M + kBlock - 1) / kBlock;
    if (blocks > 0)
        hipLaunchKernelGGL(k_depth_points_fwd, dim3((unsigned)blocks), dim3(kBlock), 0, s, image_of(H, W, Dp, ch, render, alpha), (int)M,
                           points, depths, per_point, ws);
    hipLaunchKernelGGL(k_depth_finish, dim3(1), dim3(kBlock), 0, s, blocks, ws, scale, loss, (double *)nullptr);
    return check_hip(hipGetLastError(), "depth_points_loss launch");
}

int launch_depth_points_backward(int H, int W, int Dp, int ch, const float *render, const float *alpha, int64_t M, const float *points,
                                 const float *depths, float scale, const float *upstream, float *v_render, float *v_alpha,
                                 hipStream_t s)
{
    const int64_t blocks = (M + kBlock - 1) / kBlock;
    if (blocks == 0)
        return GWBP_OK;
    const float scale_over_m = (float)((double)scale / (double)M); // float64, rounded once
    hipLaunchKernelGGL(k_depth_points_bwd, dim3((unsigned)blocks), dim3(kBlock), 0, s, image_of(H, W, Dp, ch, render, alpha), (int)M,
                       points, depths, upstream, scale_over_m, v_render, v_alpha);
    return check_hip(hipGetLastError(), "depth_points_backward launch");
}

int launch_depth_map_loss(int H, int W, int Dp, int ch, const float *render, const float *alpha, const float *depth,
                          const float *weights, int kind, float scale, float *loss, double *sums, double *ws, hipStream_t s)
{
    const int64_t pixels = (int64_t)H * W, blocks = map_blocks(pixels);
    const DepthImage I = image_of(H, W, Dp, ch, render, alpha);
    const DepthMap T{depth, weights, kind};
    with_bool(vec4_layout(Dp, render, render), [&](auto VEC4) {
        hipLaunchKernelGGL((k_depth_map_fwd<decltype(VEC4)::value>), dim3((unsigned)blocks), dim3(kBlock), 0, s, I, T, pixels, ws);
    });
    hipLaunchKernelGGL(k_depth_finish, dim3(1), dim3(kBlock), 0, s, blocks, ws, scale, loss, sums);
    return check_hip(hipGetLastError(), "depth_map_loss launch");
}

int launch_depth_map_backward(int H, int W, int Dp, int ch, const float *render, const float *alpha, const float *depth,
                              const float *weights, int kind, float scale, const double *sums, const float *upstream, float *v_render,
                              float *v_alpha, hipStream_t s)
{
    const int64_t pixels = (int64_t)H * W, blocks = map_blocks(pixels);
    const DepthImage I = image_of(H, W, Dp, ch, render, alpha);
    const DepthMap T{depth, weights, kind};
    with_bool(vec4_layout(Dp, render, v_render), [&](auto VEC4) {
        hipLaunchKernelGGL((k_depth_map_bwd<decltype(VEC4)::value>), dim3((unsigned)blocks), dim3(kBlock), 0, s, I, T, pixels, sums,
                           upstream, scale, v_render, v_alpha);
    });
    return check_hip(hipGetLastError(), "depth_map_backward launch");
}

} // namespace gwbp
