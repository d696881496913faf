// query.hip -- questions asked of a finished [N, D] feature field (the reference's segment.py / segment_compressed.py /
// click_and_segment.py: get_mask3d_lseg, and the render of the field that the click script reads one pixel of):
//
//   k_prompt_scores   s[g, j] = X[g] . prompts[j] (/ max(|X[g]|, 1e-12)),  j < P <= 32, and the 3-D mask
//                     max_{j < n_pos} s[g, j] > max_{j >= n_pos} s[g, j]  (&& s[g, 0] > threshold): ONE pass over X
//   k_probe_pixels    out[m, :] = sum_g w_g(p_m) X[g, :] at M pixels only, + the accumulated depth and alpha of those pixels
//
// ARITHMETIC CONTRACT of k_prompt_scores (the shape of k_pca_project's, pca.hip).  Every dot product AND the row's sum of squares
// is one chain of fp32 fused multiply-adds over the channel index (v_mfma_f32_16x16x4_f32 is bit for bit a k-ordered fmaf chain; the
// sum of squares is the diagonal of the row block's own 16 x 16 product, so it runs through the columns in the very order of the
// dot products), in an order that depends only on D: every chain consumes k = 32 c + 16 b + 4 q + i in the order (c, b, i, q) --
// the 32-column chunk staged per step, its 16-column block, the float4 component that feeds one MFMA, the quarter wave (the MFMA's
// k slot) -- which is knn_tile.h's order.  Columns D .. 32 ceil(D / 32) - 1 are zero-filled in LDS and their steps are executed
// (fmaf(0, 0, acc) == acc, but -0 becomes +0).  The norm is one correctly rounded sqrt, the score one correctly rounded
// divide.  Nothing depends on the row's position, on N, on P (the 16 prompts of a block are independent output columns) or on the
// launch; rows whose address and stride are 16-B aligned are read with 16-B loads, others element by element: same values, same
// chains.  Padding beyond D is never read (load4 masks it).  No atomics.  The two maxima propagate NaN as torch.max does, so a NaN
// score loses the comparison whichever side it is on.
//
// WHY NOT pca.hip's STAGING CODE.  k_pca_project subtracts the mean while it stages, stages one 16-row operand block and ends in a
// min / max reduction; here nothing is subtracted, one or two 16-prompt blocks are staged and the row block is its own second
// operand.  One shared staging routine would need a flag for the subtraction and another for the operand count inside the loop
// that decides both kernels' speed; the forty lines are kept apart and k_pca_project is not touched (its output is pinned bit for
// bit by its tests).  The prompts are staged chunk by chunk beside X (32 prompts x 2048 channels do not fit LDS at once); they
// are 256 KB at most and stay in L2.
//
// k_probe_pixels is not a second render path: it walks ONE pixel's tile list with the expressions of k_render_px (render.hip) /
// k_blend -- same sigma, exp_neg, kAlphaMin / kAlphaMax / kTMin cuts -- so its weights are the blend's bit for bit, and adds
// acc[c] = fmaf(w, X[g, c], acc[c]) front to back, the per-pixel order of k_render_px and of k_render_rows (render_wide.hip: "every
// pixel is summed front to back by its one owner").  Every loop is wave-uniform with a finite trip count (list batches, 64
// entries of a batch, the set bits of a 64-bit mask); T advances on values made uniform with v_readfirstlane.
#include "gwbp_dev.h"

namespace gwbp {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- prompt scores --------------------------------------------------------------------------------------------------------------
constexpr int kQThreads = 256; // 4 waves, each owns 32 of the workgroup's rows
constexpr int kQRows = 128;
constexpr int kQKC = 32;       // columns staged per step
constexpr int kQLd = kQKC + 4; // LDS row stride (floats): the operand reads are ds_read_b128 at 144-B steps, conflict-free per 8 lanes

// torch.max's rule: a NaN on either side is the result
__device__ __forceinline__ float max_nan(float a, float b) { return (a != a) ? a : ((b > a || b != b) ? b : a); }

// NPB: 16-prompt blocks (1: P <= 16, 2: P <= 32)
template <bool VEC, int NPB>
__global__ __launch_bounds__(kQThreads) void k_prompt_scores(int64_t N, int D, int P, int n_pos, const float *__restrict__ X,
                                                             int64_t ldx, const float *__restrict__ prompts, int normalize,
                                                             int use_thr, float thr, uint8_t *__restrict__ mask,
                                                             float *__restrict__ scores)
{
    __shared__ __attribute__((aligned(16))) float sx[2][kQRows * kQLd];
    __shared__ __attribute__((aligned(16))) float sp[2][NPB * 16 * kQLd];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = lane & 15, qd = lane >> 4;
    const int64_t q0 = (int64_t)blockIdx.x * kQRows;

    // staging role: float4 column c4 of rows r0 + 32 i (i < 4) of X, and (threads 0 .. 128 NPB - 1) of prompt r0
    const int c4 = (tid & 7) * 4, r0 = tid >> 3;
    const float *xrow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t g = q0 + r0 + 32 * i;
        xrow[i] = g < N ? X + g * ldx : nullptr;
    }
    const bool stages_p = tid < NPB * 16 * 8;
    const float *prow = (stages_p && r0 < P) ? prompts + (int64_t)r0 * D : nullptr; // a prompt beyond P stages zeros

    const int n_chunk = (D + kQKC - 1) / kQKC;
    float4 px[4], pp;
    auto prefetch = [&](int chunk) {
        const int c = chunk * kQKC + c4;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            px[i] = load4<VEC>(xrow[i], c, D);
        pp = load4<false>(prow, c, D);
    };
    prefetch(0);

    const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 acc[NPB][2]; // [pb][rb]: row 32 wave + 16 rb + m, prompts 16 pb + 4 qd + r
    f32x4 sq[2];       // [rb]: rows 16 rb + 4 qd + r against row 16 rb + m of the wave's block; the diagonal is the sum of squares
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        sq[rb] = zero;
#pragma unroll
        for (int pb = 0; pb < NPB; ++pb)
            acc[pb][rb] = zero;
    }

    for (int chunk = 0; chunk < n_chunk; ++chunk) {
        float *bx = sx[chunk & 1], *bp = sp[chunk & 1];
#pragma unroll
        for (int i = 0; i < 4; ++i) // (a row beyond N stages zeros: nothing of it is ever written)
            *reinterpret_cast<float4 *>(bx + (r0 + 32 * i) * kQLd + c4) = px[i];
        if (stages_p)
            *reinterpret_cast<float4 *>(bp + r0 * kQLd + c4) = pp;
        __syncthreads(); // (the buffers written here were last read two steps ago, before the previous barrier)
        if (chunk + 1 < n_chunk)
            prefetch(chunk + 1);

        const float *ox = bx + (wave * 32 + m) * kQLd + 4 * qd;
        const float *op = bp + m * kQLd + 4 * qd;
#pragma unroll
        for (int kb = 0; kb < kQKC / 16; ++kb) {
            float4 fp[NPB], fx[2];
#pragma unroll
            for (int pb = 0; pb < NPB; ++pb)
                fp[pb] = *reinterpret_cast<const float4 *>(op + pb * 16 * kQLd + kb * 16);
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
                fx[rb] = *reinterpret_cast<const float4 *>(ox + rb * 16 * kQLd + kb * 16);
#define GWBP_Q_STEP(E)                                                                                                \
    _Pragma("unroll") for (int rb = 0; rb < 2; ++rb)                                                                  \
    {                                                                                                                 \
        _Pragma("unroll") for (int pb = 0; pb < NPB; ++pb) acc[pb][rb] =                                              \
            __builtin_amdgcn_mfma_f32_16x16x4f32(fp[pb].E, fx[rb].E, acc[pb][rb], 0, 0, 0);                           \
        sq[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(fx[rb].E, fx[rb].E, sq[rb], 0, 0, 0);                           \
    }
            GWBP_Q_STEP(x)
            GWBP_Q_STEP(y)
            GWBP_Q_STEP(z)
            GWBP_Q_STEP(w)
#undef GWBP_Q_STEP
        }
    }

    // ---- epilogue, in registers: the row's norm, the divide, the two maxima, the compare, the byte -----------------------------
    const float ninf = -__builtin_inff();
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        const int64_t g = q0 + wave * 32 + 16 * rb + m;
        // sum of squares of row m: entry (m, m) of the block's product, held by lane (qd = m >> 2) as element m & 3
        const int e = m & 3;
        const float mine = e == 0 ? sq[rb][0] : e == 1 ? sq[rb][1] : e == 2 ? sq[rb][2] : sq[rb][3];
        const float ss = __shfl(mine, (m >> 2) * 16 + m, 64);
        const float den = __builtin_fmaxf(__builtin_sqrtf(ss), 1e-12f);
        float best_pos = ninf, best_neg = ninf, s0 = 0.f;
#pragma unroll
        for (int pb = 0; pb < NPB; ++pb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = 16 * pb + 4 * qd + r;
                const float dot = acc[pb][rb][r];
                const float s = normalize ? dot / den : dot;
                if (j < P) {
                    if (scores && g < N)
                        scores[g * P + j] = s;
                    if (j < n_pos)
                        best_pos = max_nan(best_pos, s);
                    else
                        best_neg = max_nan(best_neg, s);
                }
                if (pb == 0 && r == 0)
                    s0 = s; // (lanes qd = 0: prompt 0)
            }
        // the four lanes of a row (qd = 0 .. 3) hold its prompts 4 qd .. 4 qd + 3 of each block
        best_pos = max_nan(best_pos, __shfl_xor(best_pos, 16, 64));
        best_neg = max_nan(best_neg, __shfl_xor(best_neg, 16, 64));
        best_pos = max_nan(best_pos, __shfl_xor(best_pos, 32, 64));
        best_neg = max_nan(best_neg, __shfl_xor(best_neg, 32, 64));
        if (mask && qd == 0 && g < N) {
            bool in = n_pos < P ? best_pos > best_neg : true;
            if (use_thr)
                in = in && s0 > thr;
            mask[g] = in ? 1 : 0;
        }
    }
}

// ---- probe ----------------------------------------------------------------------------------------------------------------------
constexpr int kProbeChunk = 256; // channels per wave: four per lane

__device__ __forceinline__ float uniform_f(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ float lane_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// One wave per (probe, 256-channel chunk).  Per batch of 64 list entries: lanes = entries compute sigma and alpha; the wave then
// advances T entry by entry in list order (uniform values) and leaves each entry's weight in its lane; at last the entries that
// have a weight are added front to back, lanes = channels.
template <bool VEC>
__global__ __launch_bounds__(64) void k_probe_pixels(ViewDev V, const u32 *__restrict__ tile_offsets, const u32 *__restrict__ vals,
                                                     const G2D *__restrict__ g2d, const int32_t *__restrict__ xy,
                                                     const float *__restrict__ X, int64_t ldx, int D, float *__restrict__ out,
                                                     float *__restrict__ depth, float *__restrict__ alpha_out)
{
    const int probe = (int)blockIdx.x, chunk = (int)blockIdx.y;
    const int lane = threadIdx.x;
    const int c = chunk * kProbeChunk + 4 * lane;
    const int ix = (int)uniform((u32)xy[2 * probe]), iy = (int)uniform((u32)xy[2 * probe + 1]);
    const bool inside = ix >= 0 && ix < V.W && iy >= 0 && iy < V.H;

    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float zacc = 0.f, T = 1.0f;
    if (inside) { // wave-uniform
        const int tile = (iy / kTile) * V.tile_w + ix / kTile;
        const u32 beg = uniform(tile_offsets[tile]), end = uniform(tile_offsets[tile + 1]);
        const float px = (float)ix + 0.5f, py = (float)iy + 0.5f;
        bool done = false;
        for (u32 batch = beg; batch < end && !done; batch += 64) {
            const u32 bn = min(64u, end - batch);
            u32 gid = 0;
            float alpha = 0.f, z = 0.f;
            bool ok = false;
            if ((u32)lane < bn) {
                gid = vals[batch + lane];
                const float4 *gp = reinterpret_cast<const float4 *>(g2d + gid);
                const float4 a = gp[0], b = gp[1];
                const float dx = a.x - px, dy = a.y - py;
                const float sigma = __builtin_fmaf(b.y * dx, dy, 0.5f * __builtin_fmaf(b.x * dx, dx, (b.z * dy) * dy));
                alpha = __builtin_fminf(kAlphaMax, a.z * exp_neg(-__builtin_fmaxf(sigma, 0.f)));
                ok = (sigma >= 0.f) && (alpha >= kAlphaMin);
                z = a.w;
            }
            const u64 okm = __ballot(ok);
            // T through the batch in list order; lane j keeps entry j's weight
            float wv = 0.f;
            u64 valid = 0ull;
            for (u32 j = 0; j < bn; ++j) {
                if (!((okm >> j) & 1ull))
                    continue;
                const float al = lane_f(alpha, (int)j);
                const float next_T = uniform_f(T * (1.0f - al));
                if (next_T <= kTMin) { // terminates: not counted, nothing behind it either
                    done = true;
                    break;
                }
                const float w = uniform_f(al * T);
                wv = (u32)lane == j ? w : wv;
                valid |= 1ull << j;
                T = next_T;
            }
            // front to back, lanes = channels
            const int n_valid = __popcll(valid);
            for (int i = 0; i < n_valid; ++i) {
                const int j = __ffsll((long long)valid) - 1;
                valid &= valid - 1ull;
                const float w = lane_f(wv, j);
                const u32 g = (u32)__builtin_amdgcn_readlane((int)gid, j);
                const float4 x = load4<VEC>(X + (int64_t)g * ldx, c, D);
                acc.x = __builtin_fmaf(w, x.x, acc.x);
                acc.y = __builtin_fmaf(w, x.y, acc.y);
                acc.z = __builtin_fmaf(w, x.z, acc.z);
                acc.w = __builtin_fmaf(w, x.w, acc.w);
                zacc = __builtin_fmaf(w, lane_f(z, j), zacc);
            }
        }
    }
    float *o = out + (int64_t)probe * D;
    if (c < D)
        o[c] = acc.x;
    if (c + 1 < D)
        o[c + 1] = acc.y;
    if (c + 2 < D)
        o[c + 2] = acc.z;
    if (c + 3 < D)
        o[c + 3] = acc.w;
    if (chunk == 0 && lane == 0) {
        if (depth)
            depth[probe] = zacc;
        if (alpha_out)
            alpha_out[probe] = 1.0f - T;
    }
}

bool rows_vec(const float *X, int64_t ldx) { return !(reinterpret_cast<uintptr_t>(X) & 15) && !(ldx & 3); }

} // namespace

int launch_prompt_scores(int64_t N, int D, int P, int n_pos, const float *X, int64_t ldx, const float *prompts, int normalize,
                         const float *threshold, uint8_t *mask, float *scores, hipStream_t s)
{
    if (N == 0)
        return GWBP_OK;
    const int64_t grid = (N + kQRows - 1) / kQRows;
    if (grid > 0x7FFFFFFF)
        return set_error(GWBP_EINVAL, "prompt_scores: %lld rows need more than 2^31 - 1 workgroups", (long long)N);
    const int use_thr = threshold ? 1 : 0;
    const float thr = threshold ? *threshold : 0.f;
    const bool vec = rows_vec(X, ldx);
#define GWBP_Q(VEC, NPB)                                                                                              \
    hipLaunchKernelGGL((k_prompt_scores<VEC, NPB>), dim3((unsigned)grid), dim3(kQThreads), 0, s, N, D, P, n_pos, X, ldx, prompts, \
                       normalize, use_thr, thr, mask, scores)
    if (P <= 16) {
        if (vec)
            GWBP_Q(true, 1);
        else
            GWBP_Q(false, 1);
    } else {
        if (vec)
            GWBP_Q(true, 2);
        else
            GWBP_Q(false, 2);
    }
#undef GWBP_Q
    return check_hip(hipGetLastError(), "prompt_scores launch");
}

int launch_probe_pixels(const Ws &W, const ViewDev &V, int M, const int32_t *xy, const float *X, int64_t ldx, int D, float *out,
                        float *depth, float *alpha, hipStream_t s)
{
    const int n_tiles = V.tile_w * V.tile_h;
    const int fin = sort_passes(n_tiles) & 1;
    const dim3 grid((unsigned)M, (unsigned)((D + kProbeChunk - 1) / kProbeChunk));
    if (rows_vec(X, ldx))
        hipLaunchKernelGGL(k_probe_pixels<true>, grid, dim3(64), 0, s, V, W.tile_offsets, W.vals[fin], W.g2d, xy, X, ldx, D, out, depth,
                           alpha);
    else
        hipLaunchKernelGGL(k_probe_pixels<false>, grid, dim3(64), 0, s, V, W.tile_offsets, W.vals[fin], W.g2d, xy, X, ldx, D, out, depth,
                           alpha);
    return check_hip(hipGetLastError(), "probe_pixels launch");
}

} // namespace gwbp
