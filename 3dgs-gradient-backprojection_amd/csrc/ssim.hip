// ssim.hip -- the photometric loss of 3DGS training, (1 - lambda) L1 + lambda (1 - SSIM), of a render x against a target y, both
// float32 [H, W, D] channel-last with their own pixel strides, and its gradient with respect to x.  DESIGN.md 4 carries the contract;
// ssim_math.h carries every expression that is not a memory access.
//
//   k_ssim_fwd     one workgroup per tile of TY x TX = 16 x 64 pixels of the image, channels one after the other (a workgroup-uniform
//                  loop).  Per channel: the tile and its 5-pixel halo of x and y go to LDS (zeros outside the image); the horizontal
//                  chains of the five fields x, y, x x, y y, x y go to LDS for the tile's 26 rows; every thread runs the vertical
//                  chains of its 4 pixels (one column, 4 consecutive rows: the 14 rows it reads serve all four) and evaluates
//                  ssim_point.  It stores the SSIM map when asked for, and with want_grad the three maps w dmu, w d1, w d12 -- zero
//                  where the pixel is no window -- as PLANES [3][D][H][W] of the workspace: a lane per column, coalesced, here and when
//                  k_ssim_bwd reads them.  The tile's five float64 partial sums go to the workspace.
//   k_ssim_reduce  adds the tiles' partials in ascending tile order (a thread per sum; the partials pass through LDS) and writes the
//                  table.
//   k_ssim_bwd     the same tiling and the same two chains over the three planes, then ssim_grad and one store of v_x.  It reads Wv
//                  and Wa from the table on the device.
//
// A chain is a property of its output pixel: 11 fused multiply-adds in ascending tap order from +0 over values that are +0 outside the
// image, whatever the tile.  A tile covers pixels of the FULL image under both paddings; "valid" only masks the windows that are not
// wholly inside, so the map of a crop is the crop of the map, bit for bit.  No atomics: two runs give the same bits.
//
// LDS (static, per workgroup): forward 2 x 26 x 75 + 5 x 26 x 65 + 16 x 65 floats = 53.7 KB, backward 3 x 26 x 75 + 3 x 26 x 65 +
// 16 x 65 floats = 47.9 KB.  Row strides 75 and 65 are odd: the b32 reads and writes of a wave are 64 consecutive columns of one row
// (conflict-free at any stride), and the rows of the staging loop, which change inside a wave, start on different banks.
// Every loop is workgroup-uniform; bounds inside them are lane masks.  Every store is a vector store.
#include "gwbp_dev.h"
#include "ssim_math.h"

namespace gwbp {

namespace {

constexpr int TY = GWBP_SSIM_TILE_Y, TX = GWBP_SSIM_TILE_X;
constexpr int RY = TY + 2 * kSsimHalo, RX = TX + 2 * kSsimHalo; // the staged region: 26 x 74
constexpr int LDX = RX + 1, LDH = TX + 1;                       // LDS row strides (odd)
constexpr int kSums = 5;                                         // w ssim, w |x - y|, w (x - y)^2, Wv, Wa
constexpr int kReduceChunk = 1024;                               // tiles whose partials pass through LDS at once
static_assert(TX == 64 && TY == 16, "the thread mapping below is written for 16 x 64 tiles and 256 threads");

__constant__ float c_win[kSsimWin] = GWBP_SSIM_WINDOW;

struct SsimArgs { // wave-uniform
    int H, W, D, same;
    const float *x, *y;
    int64_t xs, ys; // pixel strides in elements; a row is W pixels
    PixW pw;
    int has_pw;
};

__device__ __forceinline__ float weight_at(const SsimArgs &A, int gy, int gx)
{
    if (!A.has_pw)
        return 1.0f;
    const int64_t off = (int64_t)gy * A.pw.ws_y + (int64_t)gx * A.pw.ws_x;
    switch (A.pw.dtype) {
    case GWBP_PIXW_U8: return static_cast<const unsigned char *>(A.pw.data)[off] != 0 ? 1.0f : 0.0f;
    case GWBP_PIXW_F16: return MapElem<GWBP_MAP_F16>::cvt(static_cast<const unsigned short *>(A.pw.data)[off]);
    case GWBP_PIXW_BF16: return MapElem<GWBP_MAP_BF16>::cvt(static_cast<const unsigned short *>(A.pw.data)[off]);
    default: return static_cast<const float *>(A.pw.data)[off];
    }
}

// the tile's weights (zero outside the image); the caller's barrier makes them visible
__device__ __forceinline__ void stage_weights(const SsimArgs &A, int oy, int ox, float *wt)
{
    for (int idx = threadIdx.x; idx < TY * TX; idx += 256) {
        const int r = idx >> 6, cx = idx & 63;
        const int gy = oy + r, gx = ox + cx;
        wt[r * LDH + cx] = gy < A.H && gx < A.W ? weight_at(A, gy, gx) : 0.0f;
    }
}

// channel c of the tile's 26 x 74 region of a channel-last image, zeros outside the image
__device__ __forceinline__ void stage_strided(const float *__restrict__ img, int64_t ps, int c, int H, int W, int oy, int ox, float *dst)
{
    for (int idx = threadIdx.x; idx < RY * RX; idx += 256) {
        const int r = idx / RX, cc = idx - r * RX;
        const int gy = oy - kSsimHalo + r, gx = ox - kSsimHalo + cc;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
        dst[r * LDX + cc] = in ? img[((int64_t)gy * W + gx) * ps + c] : 0.0f;
    }
}

// the vertical chains of the thread's 4 pixels (column tx, rows ty0 .. ty0 + 3) over one field's horizontal results
__device__ __forceinline__ void vertical4(const float *__restrict__ h, int ty0, int tx, float m[4])
{
    float col[TY / 4 + 2 * kSsimHalo];
#pragma unroll
    for (int j = 0; j < 4 + 2 * kSsimHalo; ++j)
        col[j] = h[(ty0 + j) * LDH + tx];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < kSsimWin; ++j)
            acc = ssim_chain(c_win[j], col[o + j], acc);
        m[o] = acc;
    }
}

__global__ __launch_bounds__(256) void k_ssim_fwd(SsimArgs A, float *__restrict__ planes, float *__restrict__ map_out,
                                                  double *__restrict__ partial)
{
    __shared__ float xs[RY * LDX], ys[RY * LDX];
    __shared__ float hs[5 * RY * LDH];
    __shared__ float wt[TY * LDH];
    __shared__ double red[4][kSums];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ox = (int)blockIdx.x * TX, oy = (int)blockIdx.y * TY;
    const int tx = lane, ty0 = wave * 4;
    const int gx = ox + tx;
    const int off = A.same ? 0 : kSsimHalo; // the map's origin in the image
    const int Wm = A.W - 2 * off;
    const int64_t HW = (int64_t)A.H * A.W;

    stage_weights(A, oy, ox, wt);
    double sum[kSums] = {0.0, 0.0, 0.0, 0.0, 0.0};

    for (int c = 0; c < A.D; ++c) {
        __syncthreads(); // the previous channel's readers are done
        stage_strided(A.x, A.xs, c, A.H, A.W, oy, ox, xs);
        stage_strided(A.y, A.ys, c, A.H, A.W, oy, ox, ys);
        __syncthreads();
        for (int idx = tid; idx < RY * TX; idx += 256) { // horizontal chains: a wave per row
            const int r = idx >> 6, cx = idx & 63;
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
#pragma unroll
            for (int i = 0; i < kSsimWin; ++i) {
                const float xv = xs[r * LDX + cx + i], yv = ys[r * LDX + cx + i], g = c_win[i];
                a0 = ssim_chain(g, xv, a0);
                a1 = ssim_chain(g, yv, a1);
                a2 = ssim_chain(g, xv * xv, a2);
                a3 = ssim_chain(g, yv * yv, a3);
                a4 = ssim_chain(g, xv * yv, a4);
            }
            float *h = hs + r * LDH + cx;
            h[0] = a0, h[RY * LDH] = a1, h[2 * RY * LDH] = a2, h[3 * RY * LDH] = a3, h[4 * RY * LDH] = a4;
        }
        __syncthreads();
        float m[5][4];
#pragma unroll
        for (int k = 0; k < 5; ++k)
            vertical4(hs + k * RY * LDH, ty0, tx, m[k]);
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const int gy = oy + ty0 + o;
            const bool in = gy < A.H && gx < A.W;
            const bool win = in && (A.same || (gy >= kSsimHalo && gy < A.H - kSsimHalo && gx >= kSsimHalo && gx < A.W - kSsimHalo));
            const SsimPoint P = ssim_point(m[0][o], m[1][o], m[2][o], m[3][o], m[4][o]);
            const float w = wt[(ty0 + o) * LDH + tx];
            const float xv = xs[(ty0 + o + kSsimHalo) * LDX + tx + kSsimHalo], yv = ys[(ty0 + o + kSsimHalo) * LDX + tx + kSsimHalo];
            const float e = xv - yv;
            if (win) {
                sum[0] += (double)w * (double)P.ssim;
                if (map_out)
                    map_out[((int64_t)(gy - off) * Wm + (gx - off)) * A.D + c] = P.ssim;
            }
            if (in) {
                sum[1] += (double)w * (double)__builtin_fabsf(e);
                sum[2] += (double)w * (double)(e * e);
                if (c == 0) {
                    sum[3] += win ? (double)w : 0.0;
                    sum[4] += (double)w;
                }
                if (planes) {
                    float *q = planes + (int64_t)c * HW + (int64_t)gy * A.W + gx;
                    q[0] = win ? w * P.dmu : 0.0f;
                    q[(int64_t)A.D * HW] = win ? w * P.d1 : 0.0f;
                    q[2 * (int64_t)A.D * HW] = win ? w * P.d12 : 0.0f;
                }
            }
        }
    }

#pragma unroll
    for (int k = 0; k < kSums; ++k) {
        double v = sum[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
            v += __shfl_xor(v, o, 64); // (the operands commute: every lane gets the same bits)
        if (lane == 0)
            red[wave][k] = v;
    }
    __syncthreads();
    if (tid < kSums) {
        const int64_t tile = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
        partial[tile * kSums + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
    }
}

// table = sum w ssim, sum w |x - y|, sum w (x - y)^2, Wv, Wa, windows, H W, D: the tiles' partials in ascending tile order
__global__ __launch_bounds__(256) void k_ssim_reduce(int64_t tiles, const double *__restrict__ partial, double windows, double pixels,
                                                     double D, double *__restrict__ table)
{
    __shared__ double buf[kReduceChunk * kSums];
    double s = 0.0;
    for (int64_t t0 = 0; t0 < tiles; t0 += kReduceChunk) {
        const int n = (int)min((int64_t)kReduceChunk, tiles - t0) * kSums;
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += 256)
            buf[i] = partial[t0 * kSums + i];
        __syncthreads();
        if (threadIdx.x < kSums)
            for (int i = (int)threadIdx.x; i < n; i += kSums)
                s += buf[i];
    }
    if (threadIdx.x < kSums)
        table[threadIdx.x] = s;
    if (threadIdx.x == kSums)
        table[5] = windows, table[6] = pixels, table[7] = D;
}

__global__ __launch_bounds__(256) void k_ssim_bwd(SsimArgs A, const float *__restrict__ planes, const double *__restrict__ table,
                                                  float lambda, float *__restrict__ grad, int64_t gs)
{
    __shared__ float ms[3 * RY * LDX];
    __shared__ float hs[3 * RY * LDH];
    __shared__ float wt[TY * LDH];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ox = (int)blockIdx.x * TX, oy = (int)blockIdx.y * TY;
    const int tx = lane, ty0 = wave * 4;
    const int gx = ox + tx;
    const int64_t HW = (int64_t)A.H * A.W;

    // s_s = -lambda / (D Wv), s_1 = (1 - lambda) / (D Wa) in float64, rounded once; a term whose weight sum is 0 contributes 0
    const double Wv = table[3], Wa = table[4], lam = (double)lambda;
    const float s_s = Wv != 0.0 ? (float)(-lam / ((double)A.D * Wv)) : 0.0f;
    const float s_1 = Wa != 0.0 ? (float)((1.0 - lam) / ((double)A.D * Wa)) : 0.0f;

    stage_weights(A, oy, ox, wt);
    for (int c = 0; c < A.D; ++c) {
        __syncthreads();
        for (int idx = tid; idx < RY * RX; idx += 256) { // the three planes' regions, zeros outside the image
            const int r = idx / RX, cc = idx - r * RX;
            const int gy = oy - kSsimHalo + r, px = ox - kSsimHalo + cc;
            const bool in = gy >= 0 && gy < A.H && px >= 0 && px < A.W;
            const float *q = planes + (in ? (int64_t)c * HW + (int64_t)gy * A.W + px : 0);
            ms[r * LDX + cc] = in ? q[0] : 0.0f;
            ms[RY * LDX + r * LDX + cc] = in ? q[(int64_t)A.D * HW] : 0.0f;
            ms[2 * RY * LDX + r * LDX + cc] = in ? q[2 * (int64_t)A.D * HW] : 0.0f;
        }
        __syncthreads();
        for (int idx = tid; idx < RY * TX; idx += 256) {
            const int r = idx >> 6, cx = idx & 63;
            float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
            for (int i = 0; i < kSsimWin; ++i) {
                const float g = c_win[i];
                a0 = ssim_chain(g, ms[r * LDX + cx + i], a0);
                a1 = ssim_chain(g, ms[RY * LDX + r * LDX + cx + i], a1);
                a2 = ssim_chain(g, ms[2 * RY * LDX + r * LDX + cx + i], a2);
            }
            float *h = hs + r * LDH + cx;
            h[0] = a0, h[RY * LDH] = a1, h[2 * RY * LDH] = a2;
        }
        __syncthreads();
        float m[3][4];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            vertical4(hs + k * RY * LDH, ty0, tx, m[k]);
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const int gy = oy + ty0 + o;
            if (gy < A.H && gx < A.W) {
                const int64_t p = (int64_t)gy * A.W + gx;
                const float xv = A.x[p * A.xs + c], yv = A.y[p * A.ys + c];
                grad[p * gs + c] = ssim_grad(xv, yv, wt[(ty0 + o) * LDH + tx], m[0][o], m[1][o], m[2][o], s_s, s_1);
            }
        }
    }
}

int64_t tiles_of(int H, int W) { return (int64_t)((H + TY - 1) / TY) * ((W + TX - 1) / TX); }

} // namespace

size_t image_loss_workspace_bytes(int H, int W, int D, int want_grad)
{
    return (size_t)tiles_of(H, W) * kSums * sizeof(double) + (want_grad ? (size_t)3 * H * W * D * sizeof(float) : 0);
}

int launch_image_loss(int H, int W, int D, const float *x, int64_t xs, const float *y, int64_t ys, const PixW *pw, int same,
                      float lambda, float *map, float *grad, int64_t gs, double *table, void *ws, hipStream_t s)
{
    const int64_t tiles = tiles_of(H, W);
    double *partial = static_cast<double *>(ws);
    float *planes = grad ? reinterpret_cast<float *>(partial + tiles * kSums) : nullptr;
    const int off = same ? 0 : kSsimHalo;
    const double windows = (double)(H - 2 * off) * (double)(W - 2 * off);

    SsimArgs A;
    A.H = H, A.W = W, A.D = D, A.same = same;
    A.x = x, A.y = y, A.xs = xs, A.ys = ys;
    A.has_pw = pw != nullptr;
    A.pw = pw ? *pw : PixW{nullptr, 0, 0, GWBP_PIXW_F32};
    const dim3 grid((unsigned)((W + TX - 1) / TX), (unsigned)((H + TY - 1) / TY));
    hipLaunchKernelGGL(k_ssim_fwd, grid, dim3(256), 0, s, A, planes, map, partial);
    hipLaunchKernelGGL(k_ssim_reduce, dim3(1), dim3(256), 0, s, tiles, partial, windows, (double)H * W, (double)D, table);
    if (grad)
        hipLaunchKernelGGL(k_ssim_bwd, grid, dim3(256), 0, s, A, planes, table, lambda, grad, gs);
    return check_hip(hipGetLastError(), "image_loss launch");
}

} // namespace gwbp
