// decode_loss.hip -- the part of a decoded-field training step that lies between the render of the latent table and the scatter
// of its gradient: decode, compare, and the gradients back through the decoder, without any [P, D] image.
//
//   y[p, j] = sum_k R[p, k] C[k, j]        e = y - M[p, j]        g = w_p sign(e)  (l1)   |   g = w_p (e + e)  (l2),   w_p = s c_p
//   loss = sum w_p |e|  |  sum w_p e^2      GR[p, :] = sum_j g[p, j] C[:, j]      GC[k, j] = sum_p R[p, k] g[p, j]
//
// R [P, d] are the rendered latent rows (P = H W pixels, row-major), C [d, D] the decoder, M the view's map (fp32 / fp16 / bf16
// as stored, unit channel stride, any non-negative pixel strides), c_p an optional per-pixel weight map.  d = 16 ND, ND = 1..8;
// D % 16 == 0, D <= 2048 (checked in capi.hip).
//
// TWO KERNELS derive g by the same chain, so neither stores it (four GEMM-sized products instead of three, no [P, D] buffer and no
// read-modify-write of partial sums):
//   k_decode_gc  (runs FIRST: it reads R, which GR may alias)  one workgroup per PIXEL SLICE.  It scans the slice's map rows once
//                for non-finite values (bits in LDS), then walks the 64-channel chunks of C one after the other: the wave's 16
//                columns of the chunk stay in registers, the slice's 64-pixel blocks of R pass through LDS, GC[d x 64] stays in
//                accumulators for the whole slice and is written ONCE, to the slice's partial.  It also sums the loss.
//   k_decode_gr  one workgroup per 64-pixel block, a wave per 16 pixels whose R rows stay in registers; the chunks of C pass
//                through LDS; the d / 16 accumulator tiles of GR stay resident across the chunks.
//   k_decode_reduce / k_decode_table  add the slices' partials in ascending slice order in float64.
//
// ARITHMETIC CONTRACT.  Every product sum is ONE chain of fp32 fused multiply-adds on v_mfma_f32_16x16x4_f32 (bit for bit a
// k-ordered fmaf chain from +0), in an order that depends on (d, D) and the slice plan alone:
//   y   over k: for b = 0 .. d/16 - 1, for s = 0 .. 3:  k = 16 b + s, 16 b + 4 + s, 16 b + 8 + s, 16 b + 12 + s   (chain length d)
//       -- the same chain in both kernels (the operands only swap sides), so both see the same e, the same sign, the same g.
//   GR  over j: chunks ascending, inside a chunk for t = 0 .. 3, for r = 0 .. 3:  j = 64 c + 16 t + r + 0, 4, 8, 12   (length D)
//   GC  over the slice's pixels: blocks ascending, inside a block for u = 0 .. 3, for r = 0 .. 3: pixel 16 u + r + 0, 4, 8, 12
//       (length = the slice's rows); the slices' fp32 partials are added in ascending order in float64, rounded to fp32 once.
//   loss: a lane adds its 16 terms of a (block, chunk) in fp32 (u, then r, ascending), these sums in float64; the lanes by an
//       xor butterfly (32 .. 1), the waves as (0 + 1) + (2 + 3), the slices ascending: all float64.
// The SLICE PLAN depends on P alone: 64-pixel blocks, ceil(blocks / 512) blocks per slice.  No atomics; two runs give the same
// bits.  The workspace holds 512 slice partials whatever P is.
//
// A pixel whose map row holds a non-finite value contributes nothing to loss, GR or GC, gets a zero GR row and counts in n_bad
// (field_compare.hip's convention).  k_decode_gc knows them before it starts (its scan); k_decode_gr finds them while it walks
// the chunks and zeroes the row at the end (what a bad pixel added stays in its own column of the accumulators).
//
// Every loop is workgroup-uniform (blocks, chunks, tiles); bounds inside them are lane masks.  Every store is a vector store.
#include "gwbp_dev.h"

namespace gwbp {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kSlices = GWBP_DECODE_MAX_SLICES;
constexpr int kMaxBps = GWBP_DECODE_MAX_PIXELS / 64 / kSlices; // blocks per slice at most: their bad-row bits live in LDS
constexpr int kLdC = 68; // LDS row stride of a staged chunk of C: 16-B reads of 4 columns of rows m = 0..15 fall on 16 distinct
                         // 16-B slots (68 / 4 odd); the b32 reads of rows 4 qd + s are 16 qd + 4 s + m (mod 32): distinct per half wave

struct DecArgs { // wave-uniform
    int P, W, D;
    const float *R;
    int64_t ldr;
    const float *C;
    int64_t ldc;
    const void *map;
    int64_t ms_y, ms_x;
    PixW pw;
    int mt, has_pw, l2, bps;
    int rvec, cvec, mvec; // 16-B loads of R / C rows, four-element loads of the map: where addresses and strides allow them
    float s;
};

__device__ __forceinline__ bool nonfinite(float x) { return (__float_as_uint(x) & 0x7F800000u) == 0x7F800000u; }

__device__ __forceinline__ int64_t pixel_offset(int p, int W, int64_t sy, int64_t sx)
{
    const int y = p / W;
    return (int64_t)y * sy + (int64_t)(p - y * W) * sx;
}

__device__ __forceinline__ float4 row4(const float *__restrict__ q, int vec)
{
    if (vec)
        return *reinterpret_cast<const float4 *>(q);
    return make_float4(q[0], q[1], q[2], q[3]);
}

// four / one map elements from element offset `off` on, widened to fp32
__device__ __forceinline__ float4 map4(const DecArgs &A, int64_t off)
{
    switch (A.mt) {
    case GWBP_MAP_F32:
        return row4(static_cast<const float *>(A.map) + off, A.mvec);
    case GWBP_MAP_F16: {
        typedef MapElem<GWBP_MAP_F16> E;
        const unsigned short *q = static_cast<const unsigned short *>(A.map) + off;
        if (A.mvec)
            return E::cvt4(*reinterpret_cast<const uint2 *>(q));
        return make_float4(E::cvt(q[0]), E::cvt(q[1]), E::cvt(q[2]), E::cvt(q[3]));
    }
    default: {
        typedef MapElem<GWBP_MAP_BF16> E;
        const unsigned short *q = static_cast<const unsigned short *>(A.map) + off;
        if (A.mvec)
            return E::cvt4(*reinterpret_cast<const uint2 *>(q));
        return make_float4(E::cvt(q[0]), E::cvt(q[1]), E::cvt(q[2]), E::cvt(q[3]));
    }
    }
}

__device__ __forceinline__ float map1(const DecArgs &A, int64_t off)
{
    switch (A.mt) {
    case GWBP_MAP_F32: return static_cast<const float *>(A.map)[off];
    case GWBP_MAP_F16: return MapElem<GWBP_MAP_F16>::cvt(static_cast<const unsigned short *>(A.map)[off]);
    default: return MapElem<GWBP_MAP_BF16>::cvt(static_cast<const unsigned short *>(A.map)[off]);
    }
}

// w_p = s c_p of pixel p < P (one rounding); GWBP_PIXW_U8 reads any non-zero byte as 1, like the blends
__device__ __forceinline__ float pixel_scale(const DecArgs &A, int p)
{
    if (!A.has_pw)
        return A.s;
    const int64_t off = pixel_offset(p, A.W, A.pw.ws_y, A.pw.ws_x);
    float c;
    switch (A.pw.dtype) {
    case GWBP_PIXW_U8: c = static_cast<const unsigned char *>(A.pw.data)[off] != 0 ? 1.0f : 0.0f; break;
    case GWBP_PIXW_F16: c = MapElem<GWBP_MAP_F16>::cvt(static_cast<const unsigned short *>(A.pw.data)[off]); break;
    case GWBP_PIXW_BF16: c = MapElem<GWBP_MAP_BF16>::cvt(static_cast<const unsigned short *>(A.pw.data)[off]); break;
    default: c = static_cast<const float *>(A.pw.data)[off]; break;
    }
    return A.s * c;
}

// g and the loss term of one (pixel, channel): e = y - m
__device__ __forceinline__ float grad_of(float e, float w, int l2)
{
    if (l2)
        return w * (e + e);
    return w * (e > 0.f ? 1.0f : e < 0.f ? -1.0f : 0.0f); // sign(0) = 0, as torch
}
__device__ __forceinline__ float term_of(float e, float w, int l2) { return l2 ? w * (e * e) : w * __builtin_fabsf(e); }

#define GWBP_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// ---- GC and the loss: one workgroup per pixel slice ---------------------------------------------------------------------------------
template <int ND>
__global__ __launch_bounds__(256) void k_decode_gc(DecArgs A, float *__restrict__ partial, double *__restrict__ loss_part,
                                                   double *__restrict__ bad_part)
{
    constexpr int d = 16 * ND;
    constexpr int LDR = d + 4; // (d + 4) / 4 odd: the 16-B reads of rows m = 0..15 fall on 16 distinct slots; the b32 reads of rows
                               // 4 qd + r are 16 qd + (4 | 20) r + m (mod 32): distinct per half wave
    __shared__ __attribute__((aligned(16))) float Rs[64 * LDR];
    __shared__ float wsm[64];
    __shared__ unsigned short badbits[kMaxBps * 4]; // [block of the slice][wave]: bit i = pixel 16 wave + i of the block is bad
    __shared__ u64 live_s;
    __shared__ double red[4];
    __shared__ int red_bad[4];

    const int tid = threadIdx.x, lane = tid & 63, wave = (int)uniform((u32)tid >> 6);
    const int m = lane & 15, qd = lane >> 4;
    const int slice = (int)blockIdx.x;
    const int p_base = slice * A.bps * 64;
    const int nblk = min(A.bps, (A.P - p_base + 63) / 64);

    // ---- the slice's bad rows: a wave takes 16 pixels of every block, four rows at a time, 256 channels per load -----------------
    int n_bad = 0;
    for (int blk = 0; blk < nblk; ++blk) {
        u32 bits = 0u;
#pragma unroll 1
        for (int i0 = 0; i0 < 16; i0 += 4) {
            const int pq = p_base + blk * 64 + 16 * wave + i0;
            int64_t off[4];
            bool nf[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                off[q] = pq + q < A.P ? pixel_offset(pq + q, A.W, A.ms_y, A.ms_x) : -1;
                nf[q] = false;
            }
            for (int c0 = 0; c0 < A.D; c0 += 256) {
                const int c = c0 + 4 * lane;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (off[q] >= 0 && c < A.D) {
                        const float4 v = map4(A, off[q] + c);
                        nf[q] = nf[q] || nonfinite(v.x) || nonfinite(v.y) || nonfinite(v.z) || nonfinite(v.w);
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (__ballot(nf[q]) != 0ull)
                    bits |= 1u << (i0 + q);
        }
        n_bad += __popc(bits);
        if (lane == 0)
            badbits[blk * 4 + wave] = (unsigned short)bits;
    }

    double lsum = 0.0;
    const int nchunk = (A.D + 63) / 64;
    for (int ch = 0; ch < nchunk; ++ch) {
        const int j = ch * 64 + 16 * wave + m;
        const bool wave_on = ch * 64 + 16 * wave < A.D; // wave-uniform: D % 16 == 0, a tile of 16 channels is whole or absent
        float creg[ND][4];                               // C[16 b + 4 qd + s][j]: the y operand of the wave's 16 columns
#pragma unroll
        for (int b = 0; b < ND; ++b)
#pragma unroll
            for (int s = 0; s < 4; ++s)
                creg[b][s] = wave_on ? A.C[(int64_t)(16 * b + 4 * qd + s) * A.ldc + j] : 0.f;
        f32x4 acc[ND]; // lane holds GC[16 a + 4 qd + r][j]
#pragma unroll
        for (int a = 0; a < ND; ++a)
            acc[a] = f32x4{0.f, 0.f, 0.f, 0.f};

        for (int blk = 0; blk < nblk; ++blk) {
            const int p0 = p_base + blk * 64;
            __syncthreads(); // the previous block's readers are done (and, the first time, the scan's bits are written)
#pragma unroll
            for (int i = 0; i < ND; ++i) {
                const int idx = tid + 256 * i, row = idx / (4 * ND), c = 4 * (idx % (4 * ND));
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (p0 + row < A.P)
                    v = row4(A.R + (int64_t)(p0 + row) * A.ldr + c, A.rvec);
                *reinterpret_cast<float4 *>(Rs + row * LDR + c) = v;
            }
            if (tid < 64) { // wave 0: lane = pixel of the block
                const int p = p0 + tid;
                const bool live = p < A.P && !((badbits[blk * 4 + (tid >> 4)] >> (tid & 15)) & 1);
                wsm[tid] = live ? pixel_scale(A, p) : 0.f;
                const u64 lm = __ballot(live);
                if (tid == 0)
                    live_s = lm;
            }
            __syncthreads();
            if (!wave_on)
                continue; // (wave-uniform; the barriers above are reached by every wave)
            const u64 lm = uniform64(live_s);
            // the map elements of the lane's 16 (pixel, channel) pairs first: in flight beside the y products
            float mv[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int pl = 16 * u + 4 * qd + r;
                    mv[u][r] = (lm >> pl) & 1 ? map1(A, pixel_offset(p0 + pl, A.W, A.ms_y, A.ms_x) + j) : 0.f;
                }
            float t = 0.f;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                f32x4 y = f32x4{0.f, 0.f, 0.f, 0.f}; // lane holds y[16 u + 4 qd + r][j]
#pragma unroll
                for (int b = 0; b < ND; ++b) {
                    const float4 a4 = *reinterpret_cast<const float4 *>(Rs + (16 * u + m) * LDR + 16 * b + 4 * qd);
                    y = GWBP_MFMA(a4.x, creg[b][0], y);
                    y = GWBP_MFMA(a4.y, creg[b][1], y);
                    y = GWBP_MFMA(a4.z, creg[b][2], y);
                    y = GWBP_MFMA(a4.w, creg[b][3], y);
                }
                float g[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int pl = 16 * u + 4 * qd + r;
                    const bool live = (lm >> pl) & 1;
                    const float e = y[r] - mv[u][r], w = wsm[pl];
                    g[r] = live ? grad_of(e, w, A.l2) : 0.f;
                    t += live ? term_of(e, w, A.l2) : 0.f;
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float *ra = Rs + (16 * u + 4 * qd + r) * LDR + m;
#pragma unroll
                    for (int a = 0; a < ND; ++a)
                        acc[a] = GWBP_MFMA(ra[16 * a], g[r], acc[a]);
                }
            }
            lsum += (double)t;
        }
        if (wave_on) {
            float *out = partial + (int64_t)slice * d * A.D + j;
#pragma unroll
            for (int a = 0; a < ND; ++a)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    out[(int64_t)(16 * a + 4 * qd + r) * A.D] = acc[a][r];
        }
    }

#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        lsum += __shfl_xor(lsum, o, 64); // (the operands commute: every lane gets the same bits)
    if (lane == 0) {
        red[wave] = lsum;
        red_bad[wave] = n_bad;
    }
    __syncthreads();
    if (tid == 0) {
        loss_part[slice] = (red[0] + red[1]) + (red[2] + red[3]);
        bad_part[slice] = (double)(red_bad[0] + red_bad[1] + red_bad[2] + red_bad[3]);
    }
}

// ---- GR: one workgroup per 64-pixel block, a wave per 16 pixels -------------------------------------------------------------------
template <int ND>
__global__ __launch_bounds__(256) void k_decode_gr(DecArgs A, float *GR, int64_t ldg, int gvec) // (GR may alias A.R: no __restrict__)
{
    constexpr int d = 16 * ND;
    __shared__ __attribute__((aligned(16))) float Cs[d * kLdC];

    const int tid = threadIdx.x, lane = tid & 63, wave = (int)uniform((u32)tid >> 6);
    const int m = lane & 15, qd = lane >> 4;
    const int p = (int)blockIdx.x * 64 + 16 * wave + m;
    const bool inb = p < A.P;

    // the lane's pixel: its R row (the k slots 16 b + 4 qd + s of every y product), its weight, its map row.  The wave reads its 16
    // rows of R here and writes the same 16 rows of GR at the end: GR may be R.
    float4 rreg[ND];
#pragma unroll
    for (int b = 0; b < ND; ++b)
        rreg[b] = inb ? row4(A.R + (int64_t)p * A.ldr + 16 * b + 4 * qd, A.rvec) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float w = inb ? pixel_scale(A, p) : 0.f;
    const int64_t moff = inb ? pixel_offset(p, A.W, A.ms_y, A.ms_x) : 0;

    f32x4 acc[ND]; // lane holds GR[p][16 a + 4 qd + r]
#pragma unroll
    for (int a = 0; a < ND; ++a)
        acc[a] = f32x4{0.f, 0.f, 0.f, 0.f};
    bool bad = false;

    const int nchunk = (A.D + 63) / 64;
    for (int ch = 0; ch < nchunk; ++ch) {
        const int j0 = ch * 64;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < ND; ++i) { // rows 16 i .. 16 i + 15 of C, columns j0 .. j0 + 63 (zero beyond D)
            const int idx = tid + 256 * i, row = idx >> 4, c = 4 * (idx & 15);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (j0 + c < A.D)
                v = row4(A.C + (int64_t)row * A.ldc + j0 + c, A.cvec);
            *reinterpret_cast<float4 *>(Cs + row * kLdC + c) = v;
        }
        __syncthreads();
        const int nt = min(4, (A.D - j0) / 16);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (t >= nt) // workgroup-uniform
                continue;
            const float4 mq = inb ? map4(A, moff + j0 + 16 * t + 4 * qd) : make_float4(0.f, 0.f, 0.f, 0.f);
            f32x4 y = f32x4{0.f, 0.f, 0.f, 0.f}; // lane holds y[p][j0 + 16 t + 4 qd + r]
            const float *ca = Cs + 4 * qd * kLdC + 16 * t + m;
#pragma unroll
            for (int b = 0; b < ND; ++b) {
                y = GWBP_MFMA(ca[(16 * b + 0) * kLdC], rreg[b].x, y);
                y = GWBP_MFMA(ca[(16 * b + 1) * kLdC], rreg[b].y, y);
                y = GWBP_MFMA(ca[(16 * b + 2) * kLdC], rreg[b].z, y);
                y = GWBP_MFMA(ca[(16 * b + 3) * kLdC], rreg[b].w, y);
            }
            const float mv[4] = {mq.x, mq.y, mq.z, mq.w};
            float g[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool nf = nonfinite(mv[r]);
                bad = bad || nf;
                g[r] = nf ? 0.f : grad_of(y[r] - mv[r], w, A.l2);
            }
#pragma unroll
            for (int a = 0; a < ND; ++a) {
                const float4 c4 = *reinterpret_cast<const float4 *>(Cs + (16 * a + m) * kLdC + 16 * t + 4 * qd);
                acc[a] = GWBP_MFMA(c4.x, g[0], acc[a]);
                acc[a] = GWBP_MFMA(c4.y, g[1], acc[a]);
                acc[a] = GWBP_MFMA(c4.z, g[2], acc[a]);
                acc[a] = GWBP_MFMA(c4.w, g[3], acc[a]);
            }
        }
    }

    // the pixel is bad if any of the four lanes that hold its channels met a non-finite element
    const u64 bm = __ballot(bad);
    const bool badp = (((bm | (bm >> 16) | (bm >> 32) | (bm >> 48)) >> m) & 1ull) != 0ull;
    if (!inb)
        return;
    float *out = GR + (int64_t)p * ldg + 4 * qd;
#pragma unroll
    for (int a = 0; a < ND; ++a) {
        const float4 v = badp ? make_float4(0.f, 0.f, 0.f, 0.f) : make_float4(acc[a][0], acc[a][1], acc[a][2], acc[a][3]);
        if (gvec) {
            *reinterpret_cast<float4 *>(out + 16 * a) = v;
        } else {
            out[16 * a] = v.x, out[16 * a + 1] = v.y, out[16 * a + 2] = v.z, out[16 * a + 3] = v.w;
        }
    }
}

// GC[k, j] = the slices' partials added in ascending slice order in float64, rounded to fp32 once (zero slices: zero)
__global__ __launch_bounds__(256) void k_decode_reduce(int d, int D, int slices, const float *__restrict__ partial,
                                                       float *__restrict__ GC, int64_t ldgc)
{
    const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (e >= d * D)
        return;
    double s = 0.0;
    for (int i = 0; i < slices; ++i)
        s += (double)partial[(int64_t)i * d * D + e];
    GC[(int64_t)(e / D) * ldgc + e % D] = (float)s;
}

// table = loss_sum, n_pixels (not bad), n_bad, P, d, D, 0, 0
__global__ void k_decode_table(int P, int d, int D, int slices, const double *__restrict__ loss_part,
                               const double *__restrict__ bad_part, double *__restrict__ table)
{
    if (threadIdx.x != 0)
        return;
    double loss = 0.0, bad = 0.0;
    for (int i = 0; i < slices; ++i) {
        loss += loss_part[i];
        bad += bad_part[i];
    }
    table[0] = loss, table[1] = (double)P - bad, table[2] = bad, table[3] = (double)P;
    table[4] = (double)d, table[5] = (double)D, table[6] = 0.0, table[7] = 0.0;
}

bool aligned16(const void *p, int64_t ld) { return !(reinterpret_cast<uintptr_t>(p) & 15) && !(ld & 3); }

} // namespace

size_t decode_loss_workspace_bytes(int d, int D) { return (size_t)kSlices * ((size_t)d * D * sizeof(float) + 2 * sizeof(double)); }

int launch_decode_loss(int H, int W, int d, int D, const float *R, int64_t ldr, const float *C, int64_t ldc, const void *map, int mt,
                       int64_t ms_y, int64_t ms_x, const PixW *pw, int l2, float scale, float *GR, int64_t ldg, float *GC,
                       int64_t ldgc, double *table, void *ws, hipStream_t s)
{
    const int P = H * W; // <= GWBP_DECODE_MAX_PIXELS (capi.hip)
    const int nb = (P + 63) / 64;
    const int bps = nb > 0 ? (nb + kSlices - 1) / kSlices : 1;
    const int slices = (nb + bps - 1) / bps;

    float *partial = static_cast<float *>(ws);
    double *loss_part = reinterpret_cast<double *>(partial + (size_t)kSlices * d * D);
    double *bad_part = loss_part + kSlices;

    if (P > 0) {
        DecArgs A;
        A.P = P, A.W = W, A.D = D;
        A.R = R, A.ldr = ldr, A.C = C, A.ldc = ldc;
        A.map = map, A.ms_y = ms_y, A.ms_x = ms_x, A.mt = mt;
        A.has_pw = pw != nullptr;
        A.pw = pw ? *pw : PixW{nullptr, 0, 0, GWBP_PIXW_F32};
        A.l2 = l2, A.bps = bps, A.s = scale;
        A.rvec = aligned16(R, ldr), A.cvec = aligned16(C, ldc);
        A.mvec = !(reinterpret_cast<uintptr_t>(map) & (mt == GWBP_MAP_F32 ? 15 : 7)) && !(ms_y & 3) && !(ms_x & 3);
        const int gvec = aligned16(GR, ldg);
#define GWBP_DEC(N)                                                                                                                  \
    case N:                                                                                                                          \
        hipLaunchKernelGGL(k_decode_gc<N>, dim3((unsigned)slices), dim3(256), 0, s, A, partial, loss_part, bad_part);                \
        hipLaunchKernelGGL(k_decode_gr<N>, dim3((unsigned)nb), dim3(256), 0, s, A, GR, ldg, gvec);                                   \
        break
        switch (d / 16) {
            GWBP_DEC(1);
            GWBP_DEC(2);
            GWBP_DEC(3);
            GWBP_DEC(4);
            GWBP_DEC(5);
            GWBP_DEC(6);
            GWBP_DEC(7);
        default:
            GWBP_DEC(8);
        }
#undef GWBP_DEC
        const int rc = check_hip(hipGetLastError(), "decode_loss launch");
        if (rc)
            return rc;
    }
    hipLaunchKernelGGL(k_decode_reduce, dim3((unsigned)((d * D + 255) / 256)), dim3(256), 0, s, d, D, slices, partial, GC, ldgc);
    hipLaunchKernelGGL(k_decode_table, dim3(1), dim3(64), 0, s, P, d, D, slices, loss_part, bad_part, table);
    return check_hip(hipGetLastError(), "decode_loss reduce launch");
}

} // namespace gwbp
