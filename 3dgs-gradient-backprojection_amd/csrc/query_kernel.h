// query_kernel.h -- k_prompt_scores and k_probe_pixels (see query.hip for the contracts) as templates over the element type of the
// field, and their typed launchers: query.hip instantiates it for fp32 fields, query_half.hip for fp16 / bf16 ones.
#pragma once
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

// NPB: 16-prompt blocks (1: P <= 16, 2: P <= 32).  MT: the element type of X (a half field is widened as it is loaded: the staged
// values, and with them every chain, are those of the fp32 kernel on the widened field)
template <int MT, bool VEC, int NPB>
__global__ __launch_bounds__(kQThreads) void k_prompt_scores(int64_t N, int D, int P, int n_pos,
                                                             const typename MapElem<MT>::raw *__restrict__ X, int64_t ldx,
                                                             const float *__restrict__ prompts, int normalize,
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
    const typename MapElem<MT>::raw *xrow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t g = q0 + r0 + 32 * i;
        xrow[i] = g < N ? X + g * ldx : nullptr;
    }
    const bool stages_p = tid < NPB * 16 * 8;
    const float *prow = (stages_p && r0 < P) ? prompts + (int64_t)r0 * D : nullptr; // a prompt beyond P stages zeros

    const int n_chunk = (D + kQKC - 1) / kQKC;
    typename MapElem<MT>::raw4 px[4]; // (the bits as loaded: widened where the staging writes them)
    float4 pp;
    auto prefetch = [&](int chunk) {
        const int c = chunk * kQKC + c4;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            px[i] = load4raw<MT, VEC>(xrow[i], c, D);
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
            *reinterpret_cast<float4 *>(bx + (r0 + 32 * i) * kQLd + c4) = widen4<MT>(px[i]);
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

template <int MT>
void launch_prompt_scores_t(unsigned grid, hipStream_t s, int64_t N, int D, int P, int n_pos, const void *Xv, int64_t ldx,
                            const float *prompts, int normalize, int use_thr, float thr, uint8_t *mask, float *scores)
{
    with_bool(field_rows_vec(Xv, ldx, MT), [&](auto VEC) {
        with_bool(P <= 16, [&](auto ONE) { // 16-prompt blocks: one or two
            hipLaunchKernelGGL((k_prompt_scores<MT, VEC, ONE ? 1 : 2>), dim3(grid), dim3(kQThreads), 0, s, N, D, P, n_pos,
                               field_ptr<MT>(Xv), ldx, prompts, normalize, use_thr, thr, mask, scores);
        });
    });
}

// ---- probe ----------------------------------------------------------------------------------------------------------------------
constexpr int kProbeChunk = 256; // channels per wave: four per lane

__device__ __forceinline__ float uniform_f(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ float lane_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// One wave per (probe, 256-channel chunk).  Per batch of 64 list entries: lanes = entries compute sigma and alpha; the wave then
// advances T entry by entry in list order (uniform values) and leaves each entry's weight in its lane; at last the entries that
// have a weight are added front to back, lanes = channels.
// MT: the element type of X (a half row is widened where it is loaded: the chains are those of the fp32 kernel on the widened table)
template <int MT, bool VEC>
__global__ __launch_bounds__(64) void k_probe_pixels(ViewDev V, const u32 *__restrict__ tile_offsets, const u32 *__restrict__ vals,
                                                     const G2D *__restrict__ g2d, const int32_t *__restrict__ xy,
                                                     const typename MapElem<MT>::raw *__restrict__ X, int64_t ldx, int D,
                                                     float *__restrict__ out,
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
                const float4 x = load4t<MT, VEC>(X + (int64_t)g * ldx, c, D);
                acc.x = __builtin_fmaf(w, x.x, acc.x);
                acc.y = __builtin_fmaf(w, x.y, acc.y);
                acc.z = __builtin_fmaf(w, x.z, acc.z);
                acc.w = __builtin_fmaf(w, x.w, acc.w);
                zacc = __builtin_fmaf(w, lane_f(z, j), zacc);
            }
        }
    }
    store4<false>(out + (int64_t)probe * D, c, D, acc);
    if (chunk == 0 && lane == 0) {
        if (depth)
            depth[probe] = zacc;
        if (alpha_out)
            alpha_out[probe] = 1.0f - T;
    }
}

template <int MT>
void launch_probe_pixels_t(const Ws &W, const ViewDev &V, int M, const int32_t *xy, const void *Xv, int64_t ldx, int D, float *out,
                           float *depth, float *alpha, hipStream_t s)
{
    const int n_tiles = V.tile_w * V.tile_h;
    const int fin = sort_passes(n_tiles) & 1;
    const dim3 grid((unsigned)M, (unsigned)((D + kProbeChunk - 1) / kProbeChunk));
    with_bool(field_rows_vec(Xv, ldx, MT), [&](auto VEC) {
        hipLaunchKernelGGL((k_probe_pixels<MT, VEC>), grid, dim3(64), 0, s, V, W.tile_offsets, W.vals[fin], W.g2d, xy, field_ptr<MT>(Xv),
                           ldx, D, out, depth, alpha);
    });
}

} // namespace

} // namespace gwbp
