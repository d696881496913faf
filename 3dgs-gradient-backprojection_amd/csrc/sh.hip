// sh.hip -- the SH colours of a training step and their backward.  sh_math.h carries every expression that is not a
// memory access; the forward gives k_sh_colors' bits (csrc/render.hip), the backward differentiates projection.sh_colors_torch.
//
//   k_sh_eval<DEG>      out[i] = the colour of Gaussian i from a coefficient row that is split over two tables: coefficient k is
//                       head[i][k] for k < K_head and tail[i][k - K_head] behind (tail == nullptr: one table).
//   k_sh_eval_bwd<DEG>  v_head, v_tail (the rows' gradients, exact +0 from row (DEG + 1)^2 on) and v_means from v_colors; each output
//                       may be nullptr.  It recomputes direction, basis and pre-clamp colour: the forward saves nothing.
//   k_sh_eval_dev<DEG>, k_sh_eval_bwd_dev<DEG>, k_sh_campos_sum   the same with the camera centre read on the device, and its
//                       gradient v_campos (a pose that is trained with the Gaussians); described where they stand.
//
// Memory shape.  A thread owns a Gaussian, but a lane-per-row walk of 180-B or 192-B rows would scatter every load over 64 rows.  The
// rows of a workgroup's 256 Gaussians are one contiguous span of each table: the workgroup copies the span into LDS with consecutive
// lanes on consecutive 16-B chunks (consecutive dwords when the table is not 16-B aligned; the span's offset inside its table,
// 256 rows x 12 K B x blockIdx, is a multiple of 16 B), every thread then reads its own row [3 (K_head + K_tail)] there, at a row stride
// of 3 (K_head + K_tail) | 1 dwords (odd: the 32 lanes of a ds_read_b32 group are on 32 banks).  The backward overwrites the row with its
// gradient, entry by entry behind the read, and the workgroup copies the spans out the same way.
//
// No atomics, nothing between workgroups: the result is a function of the inputs alone, the same bits every run.  Every thread reaches
// every barrier (rows >= N idle, nobody returns early), every loop bound is a kernel argument, and an index into LDS is below
// 256 x stride because row < rows <= 256 and column < 3 K.
#include "gwbp_dev.h"
#include "sh_math.h"

namespace gwbp {

namespace {

constexpr int kShBlock = 256;
constexpr int kShBatch = 6; // 16-B chunks a thread keeps in flight while it stages a span (K = 16: 12 chunks, two passes)

__host__ __device__ inline int sh_stride(int k_total) { return (3 * k_total) | 1; }

// (row, column) of element f of a span of rows of w dwords
struct ShPos {
    int row, col;
};

__device__ inline ShPos sh_pos(unsigned f, unsigned w) { return ShPos{(int)(f / w), (int)(f % w)}; }

// the span `g` (count dwords: the workgroup's rows of w dwords each) <-> LDS rows at column `at`, row stride `stride`.  OUT: LDS to g.
template <bool OUT> __device__ inline void sh_copy_span(float *g, unsigned count, unsigned w, float *lds, int at, int stride)
{
    const unsigned t = threadIdx.x;
    if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
        const unsigned n4 = count / 4;
        // kShBatch chunks per thread and pass: the loads of a pass are all issued before the first is waited for (one load per
        // pass would leave a workgroup's 12 passes at K = 16 waiting for memory one after the other)
        for (unsigned q0 = t; q0 < n4; q0 += kShBatch * kShBlock) {
            float4 v[kShBatch];
            if (!OUT) {
#pragma unroll
                for (int b = 0; b < kShBatch; ++b) {
                    const unsigned q = q0 + b * kShBlock;
                    v[b] = q < n4 ? *reinterpret_cast<const float4 *>(g + 4 * (size_t)q) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
#pragma unroll
            for (int b = 0; b < kShBatch; ++b) {
                const unsigned q = q0 + b * kShBlock;
                if (q >= n4)
                    break;
                ShPos p = sh_pos(4 * q, w);
                float e[4] = {0.f, 0.f, 0.f, 0.f};
                if (!OUT)
                    e[0] = v[b].x, e[1] = v[b].y, e[2] = v[b].z, e[3] = v[b].w;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float *cell = lds + p.row * stride + at + p.col;
                    if (OUT)
                        e[j] = *cell;
                    else
                        *cell = e[j];
                    if (++p.col == (int)w)
                        p.col = 0, ++p.row;
                }
                if (OUT)
                    *reinterpret_cast<float4 *>(g + 4 * (size_t)q) = make_float4(e[0], e[1], e[2], e[3]);
            }
        }
        for (unsigned f = 4 * n4 + t; f < count; f += kShBlock) { // (the last workgroup's span may end inside a chunk)
            const ShPos p = sh_pos(f, w);
            if (OUT)
                g[f] = lds[p.row * stride + at + p.col];
            else
                lds[p.row * stride + at + p.col] = g[f];
        }
    } else {
        for (unsigned f = t; f < count; f += kShBlock) {
            const ShPos p = sh_pos(f, w);
            if (OUT)
                g[f] = lds[p.row * stride + at + p.col];
            else
                lds[p.row * stride + at + p.col] = g[f];
        }
    }
}

template <int DEG>
__global__ __launch_bounds__(kShBlock) void k_sh_eval(int64_t N, int k_head, int k_tail, const float *__restrict__ means,
                                                      const float *head, const float *tail, float cx, float cy, float cz,
                                                      float *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) float s_rows[];
    const int64_t first = (int64_t)blockIdx.x * kShBlock;
    const int64_t left = N - first;
    const unsigned rows = left < kShBlock ? (unsigned)left : (unsigned)kShBlock;
    const int stride = sh_stride(k_head + k_tail);
    sh_copy_span<false>(const_cast<float *>(head) + (size_t)first * 3 * k_head, rows * 3u * k_head, 3u * k_head, s_rows, 0, stride);
    if (tail)
        sh_copy_span<false>(const_cast<float *>(tail) + (size_t)first * 3 * k_tail, rows * 3u * k_tail, 3u * k_tail, s_rows, 3 * k_head,
                            stride);
    __syncthreads();
    if (threadIdx.x < rows) {
        const int64_t i = first + threadIdx.x;
        const float m[3] = {means[3 * i], means[3 * i + 1], means[3 * i + 2]};
        float c[3];
        sh_forward_row<DEG>(m, cx, cy, cz, s_rows + threadIdx.x * stride, c);
        out[3 * i] = c[0], out[3 * i + 1] = c[1], out[3 * i + 2] = c[2];
    }
}

template <int DEG>
__global__ __launch_bounds__(kShBlock) void k_sh_eval_bwd(int64_t N, int k_head, int k_tail, const float *__restrict__ means,
                                                          const float *head, const float *tail, float cx, float cy, float cz,
                                                          const float *__restrict__ v_colors, float *v_head, float *v_tail,
                                                          float *__restrict__ v_means)
{
    extern __shared__ __attribute__((aligned(16))) float s_rows[];
    const int64_t first = (int64_t)blockIdx.x * kShBlock;
    const int64_t left = N - first;
    const unsigned rows = left < kShBlock ? (unsigned)left : (unsigned)kShBlock;
    const int stride = sh_stride(k_head + k_tail);
    sh_copy_span<false>(const_cast<float *>(head) + (size_t)first * 3 * k_head, rows * 3u * k_head, 3u * k_head, s_rows, 0, stride);
    if (tail)
        sh_copy_span<false>(const_cast<float *>(tail) + (size_t)first * 3 * k_tail, rows * 3u * k_tail, 3u * k_tail, s_rows, 3 * k_head,
                            stride);
    __syncthreads();
    if (threadIdx.x < rows) {
        const int64_t i = first + threadIdx.x;
        const float m[3] = {means[3 * i], means[3 * i + 1], means[3 * i + 2]};
        const float v[3] = {v_colors[3 * i], v_colors[3 * i + 1], v_colors[3 * i + 2]};
        float *row = s_rows + threadIdx.x * stride;
        float *const v_row = (v_head || v_tail) ? row : nullptr;
        if (v_means) { // (two calls: a pointer that may be null would put vm into scratch)
            float vm[3];
            sh_backward_row<DEG>(m, cx, cy, cz, row, k_head + k_tail, v, v_row, vm);
            v_means[3 * i] = vm[0], v_means[3 * i + 1] = vm[1], v_means[3 * i + 2] = vm[2];
        } else {
            sh_backward_row<DEG>(m, cx, cy, cz, row, k_head + k_tail, v, v_row, nullptr);
        }
    }
    __syncthreads();
    if (v_head)
        sh_copy_span<true>(v_head + (size_t)first * 3 * k_head, rows * 3u * k_head, 3u * k_head, s_rows, 0, stride);
    if (v_tail)
        sh_copy_span<true>(v_tail + (size_t)first * 3 * k_tail, rows * 3u * k_tail, 3u * k_tail, s_rows, 3 * k_head, stride);
}

// ---- the centre on the device, and its gradient ------------------------------------------------------------------------------------
// k_sh_eval_dev / k_sh_eval_bwd_dev are the two kernels above with `campos` a device pointer to three floats: every thread loads
// them (one address for the whole grid), everything behind the loads is the same expression, so the same three values give the same
// bits.  The backward adds v_campos: dir = mean - campos, so d loss / d campos = -sum_i vm_i over the rows' float32 v_means values.
// The sum follows project_grad.hip: each thread widens its three values to double (rows >= N hold exact 0), the lanes of a wave are
// added by shuffles, the waves of a block in LDS in wave order, each block stores its [3] with plain stores into the caller's scratch
// [n_blocks, 3], and k_sh_campos_sum, one workgroup, adds the blocks in block order and negates.  No atomics: same inputs, same bits.
constexpr int kCamGrad = 3;

template <int DEG>
__global__ __launch_bounds__(kShBlock) void k_sh_eval_dev(int64_t N, int k_head, int k_tail, const float *__restrict__ means,
                                                          const float *head, const float *tail, const float *__restrict__ campos,
                                                          float *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) float s_rows[];
    const float cx = campos[0], cy = campos[1], cz = campos[2];
    const int64_t first = (int64_t)blockIdx.x * kShBlock;
    const int64_t left = N - first;
    const unsigned rows = left < kShBlock ? (unsigned)left : (unsigned)kShBlock;
    const int stride = sh_stride(k_head + k_tail);
    sh_copy_span<false>(const_cast<float *>(head) + (size_t)first * 3 * k_head, rows * 3u * k_head, 3u * k_head, s_rows, 0, stride);
    if (tail)
        sh_copy_span<false>(const_cast<float *>(tail) + (size_t)first * 3 * k_tail, rows * 3u * k_tail, 3u * k_tail, s_rows, 3 * k_head,
                            stride);
    __syncthreads();
    if (threadIdx.x < rows) {
        const int64_t i = first + threadIdx.x;
        const float m[3] = {means[3 * i], means[3 * i + 1], means[3 * i + 2]};
        float c[3];
        sh_forward_row<DEG>(m, cx, cy, cz, s_rows + threadIdx.x * stride, c);
        out[3 * i] = c[0], out[3 * i + 1] = c[1], out[3 * i + 2] = c[2];
    }
}

template <int DEG>
__global__ __launch_bounds__(kShBlock) void k_sh_eval_bwd_dev(int64_t N, int k_head, int k_tail, const float *__restrict__ means,
                                                              const float *head, const float *tail,
                                                              const float *__restrict__ campos, const float *__restrict__ v_colors,
                                                              float *v_head, float *v_tail, float *__restrict__ v_means,
                                                              double *__restrict__ partials)
{
    extern __shared__ __attribute__((aligned(16))) float s_rows[];
    const float cx = campos[0], cy = campos[1], cz = campos[2];
    const int64_t first = (int64_t)blockIdx.x * kShBlock;
    const int64_t left = N - first;
    const unsigned rows = left < kShBlock ? (unsigned)left : (unsigned)kShBlock;
    const int stride = sh_stride(k_head + k_tail);
    sh_copy_span<false>(const_cast<float *>(head) + (size_t)first * 3 * k_head, rows * 3u * k_head, 3u * k_head, s_rows, 0, stride);
    if (tail)
        sh_copy_span<false>(const_cast<float *>(tail) + (size_t)first * 3 * k_tail, rows * 3u * k_tail, 3u * k_tail, s_rows, 3 * k_head,
                            stride);
    __syncthreads();
    float vm[3] = {0.f, 0.f, 0.f}; // (rows >= N keep the zeros and add them below)
    if (threadIdx.x < rows) {
        const int64_t i = first + threadIdx.x;
        const float m[3] = {means[3 * i], means[3 * i + 1], means[3 * i + 2]};
        const float v[3] = {v_colors[3 * i], v_colors[3 * i + 1], v_colors[3 * i + 2]};
        float *row = s_rows + threadIdx.x * stride;
        float *const v_row = (v_head || v_tail) ? row : nullptr;
        if (v_means || partials) {
            sh_backward_row<DEG>(m, cx, cy, cz, row, k_head + k_tail, v, v_row, vm);
            if (v_means)
                v_means[3 * i] = vm[0], v_means[3 * i + 1] = vm[1], v_means[3 * i + 2] = vm[2];
        } else {
            sh_backward_row<DEG>(m, cx, cy, cz, row, k_head + k_tail, v, v_row, nullptr);
        }
    }
    __syncthreads();
    if (v_head)
        sh_copy_span<true>(v_head + (size_t)first * 3 * k_head, rows * 3u * k_head, 3u * k_head, s_rows, 0, stride);
    if (v_tail)
        sh_copy_span<true>(v_tail + (size_t)first * 3 * k_tail, rows * 3u * k_tail, 3u * k_tail, s_rows, 3 * k_head, stride);

    // The centre's sums, in an LDS array of their own (s_rows may still be read by a slower wave's copy-out).  `partials` is a kernel
    // argument: the branch is uniform over the grid, and inside it every thread takes part in every shuffle and reaches the barrier.
    if (partials) {
        __shared__ double s_wave[kShBlock / 64][kCamGrad];
        double acc[kCamGrad] = {(double)vm[0], (double)vm[1], (double)vm[2]};
#pragma unroll
        for (int k = 0; k < kCamGrad; ++k)
#pragma unroll
            for (int o = 32; o > 0; o >>= 1)
                acc[k] += __shfl_down(acc[k], o, 64);
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < kCamGrad; ++k)
                s_wave[wave][k] = acc[k];
        }
        __syncthreads();
        if (threadIdx.x < kCamGrad) {
            double sum = s_wave[0][threadIdx.x];
#pragma unroll
            for (int w = 1; w < kShBlock / 64; ++w)
                sum += s_wave[w][threadIdx.x];
            partials[(int64_t)blockIdx.x * kCamGrad + threadIdx.x] = sum;
        }
    }
}

// out[k] = -(the blocks' partial sums in block order): thread (c, k) adds value k of the blocks of chunk c, first to last; after the
// barrier the chunks are added first to last.  0.0 - sum, not -sum: a sum of zeros (degree 0) gives +0.  One workgroup; every thread
// reaches the barrier.
constexpr int kCamChunks = 85; // 85 x 3 = 255 of 256 threads
__global__ __launch_bounds__(256) void k_sh_campos_sum(int n_blocks, const double *__restrict__ partials, double *__restrict__ out)
{
    __shared__ double s_chunk[kCamChunks][kCamGrad];
    const int c = threadIdx.x / kCamGrad, k = threadIdx.x % kCamGrad;
    const int per = (n_blocks + kCamChunks - 1) / kCamChunks;
    if (c < kCamChunks) {
        double sum = 0.0;
        const int begin = min(n_blocks, c * per), end = min(n_blocks, (c + 1) * per);
        for (int b = begin; b < end; ++b)
            sum += partials[(int64_t)b * kCamGrad + k];
        s_chunk[c][k] = sum;
    }
    __syncthreads();
    if (threadIdx.x < kCamGrad) {
        double sum = s_chunk[0][threadIdx.x];
        for (int j = 1; j < kCamChunks; ++j)
            sum += s_chunk[j][threadIdx.x];
        out[threadIdx.x] = 0.0 - sum;
    }
}

} // namespace

size_t sh_lds_bytes(int k_total) { return (size_t)kShBlock * sh_stride(k_total) * sizeof(float); }

int launch_sh_eval(int64_t N, int degree, int k_head, int k_tail, const float *means, const float *head, const float *tail,
                   const float *campos, float *out, hipStream_t s)
{
    unsigned grid;
    if (int rc = grid_of("sh_eval", N, &grid, kShBlock))
        return rc;
    if (grid == 0)
        return GWBP_OK;
    const size_t lds = sh_lds_bytes(k_head + k_tail);
#define GWBP_SH(D)                                                                                                                \
    hipLaunchKernelGGL(k_sh_eval<D>, dim3(grid), dim3(kShBlock), lds, s, N, k_head, k_tail, means, head, tail, campos[0], campos[1],  \
                       campos[2], out)
    switch (degree) {
    case 0: GWBP_SH(0); break;
    case 1: GWBP_SH(1); break;
    case 2: GWBP_SH(2); break;
    default: GWBP_SH(3); break;
    }
#undef GWBP_SH
    return check_hip(hipGetLastError(), "sh_eval launch");
}

int launch_sh_eval_bwd(int64_t N, int degree, int k_head, int k_tail, const float *means, const float *head, const float *tail,
                       const float *campos, const float *v_colors, float *v_head, float *v_tail, float *v_means, hipStream_t s)
{
    unsigned grid;
    if (int rc = grid_of("sh_eval_backward", N, &grid, kShBlock))
        return rc;
    if (grid == 0)
        return GWBP_OK;
    const size_t lds = sh_lds_bytes(k_head + k_tail);
#define GWBP_SH(D)                                                                                                                \
    hipLaunchKernelGGL(k_sh_eval_bwd<D>, dim3(grid), dim3(kShBlock), lds, s, N, k_head, k_tail, means, head, tail, campos[0],         \
                       campos[1], campos[2], v_colors, v_head, v_tail, v_means)
    switch (degree) {
    case 0: GWBP_SH(0); break;
    case 1: GWBP_SH(1); break;
    case 2: GWBP_SH(2); break;
    default: GWBP_SH(3); break;
    }
#undef GWBP_SH
    return check_hip(hipGetLastError(), "sh_eval_backward launch");
}

int launch_sh_eval_dev(int64_t N, int degree, int k_head, int k_tail, const float *means, const float *head, const float *tail,
                       const float *campos_dev, float *out, hipStream_t s)
{
    unsigned grid;
    if (int rc = grid_of("sh_eval_dev", N, &grid, kShBlock))
        return rc;
    if (grid == 0)
        return GWBP_OK;
    const size_t lds = sh_lds_bytes(k_head + k_tail);
#define GWBP_SH(D)                                                                                                                \
    hipLaunchKernelGGL(k_sh_eval_dev<D>, dim3(grid), dim3(kShBlock), lds, s, N, k_head, k_tail, means, head, tail, campos_dev, out)
    switch (degree) {
    case 0: GWBP_SH(0); break;
    case 1: GWBP_SH(1); break;
    case 2: GWBP_SH(2); break;
    default: GWBP_SH(3); break;
    }
#undef GWBP_SH
    return check_hip(hipGetLastError(), "sh_eval_dev launch");
}

int sh_eval_backward_blocks(int64_t n) { return (int)((n + kShBlock - 1) / kShBlock); }

int launch_sh_eval_bwd_dev(int64_t N, int degree, int k_head, int k_tail, const float *means, const float *head, const float *tail,
                           const float *campos_dev, const float *v_colors, float *v_head, float *v_tail, float *v_means,
                           double *v_campos, double *scratch, hipStream_t s)
{
    unsigned grid;
    if (int rc = grid_of("sh_eval_backward_dev", N, &grid, kShBlock))
        return rc;
    if (grid == 0) {
        if (v_campos)
            return check_hip(hipMemsetAsync(v_campos, 0, kCamGrad * sizeof(double), s), "memset v_campos");
        return GWBP_OK;
    }
    const size_t lds = sh_lds_bytes(k_head + k_tail);
#define GWBP_SH(D)                                                                                                                \
    hipLaunchKernelGGL(k_sh_eval_bwd_dev<D>, dim3(grid), dim3(kShBlock), lds, s, N, k_head, k_tail, means, head, tail, campos_dev,    \
                       v_colors, v_head, v_tail, v_means, v_campos ? scratch : nullptr)
    switch (degree) {
    case 0: GWBP_SH(0); break;
    case 1: GWBP_SH(1); break;
    case 2: GWBP_SH(2); break;
    default: GWBP_SH(3); break;
    }
#undef GWBP_SH
    if (v_campos)
        hipLaunchKernelGGL(k_sh_campos_sum, dim3(1), dim3(256), 0, s, (int)grid, scratch, v_campos);
    return check_hip(hipGetLastError(), "sh_eval_backward_dev launch");
}

} // namespace gwbp
