// pca.hip -- the [N, D] passes of a PCA of a finished feature field (the reference's visualize_pca.py: sklearn PCA(3) on the host):
//
//   k_column_sums / k_column_means   mu[c]   = (1 / N) sum_g X[g, c]
//   k_centered_gram / k_gram_reduce  G[a, b] = sum_g (X[g, a] - mu[a]) (X[g, b] - mu[b])          (float64 [D, D])
//   k_pca_project                    Y[g, j] = sum_c (X[g, c] - mu[c]) V[j, c],  j < k <= 16, + per-workgroup min / max of Y
//   k_pca_colors                     colors  = (Y - lo) / (hi - lo)
//
// The eigen-decomposition between the second and the third is a D x D problem and stays with the caller (pca.py: float64 eigh).
//
// ARITHMETIC CONTRACT.  X is read in place, fp32, with any row stride >= D; no [N, D] intermediate exists: x - mu is ONE fp32
// subtraction done while a row chunk is staged into LDS, so the Gram is the CENTRED one (lifted features share a large common
// component: the uncentred form sum x x^T - N mu mu^T loses three digits to cancellation at a mean of 5 sigma).
//   * Means: every thread sums its column over its rows of a row slice in float64, in ascending row order; the slices are
//     added in ascending order in float64; mu is that sum / N rounded to fp32 once.
//   * Gram: the rows are cut into `slices` equal runs (gram_slices: a function of N and D alone).  A workgroup owns one 128 x 128
//     tile of the upper triangle and one slice; every entry of its partial tile is ONE chain of fp32 fused multiply-adds over the
//     slice's rows (v_mfma_f32_16x16x4_f32 is bit for bit a k-ordered fmaf chain), in an order that depends only on the row's
//     offset in the slice.  Rows at or beyond N enter as 0 (not as -mu), columns at or beyond D as 0.  The partial tiles go to the
//     workspace [slices][D][D] and k_gram_reduce adds them in ascending slice order in float64 and mirrors the lower triangle.
//   * Projection: one fmaf chain per Y entry over c, in an order that depends only on D (as knn.hip's scores).
// No atomics anywhere: every result is bit-reproducible from run to run, and does not depend on alignment (rows whose addresses
// and stride are 16-B aligned are read with 16-B loads, others element by element: same values, same chains).
//
// Every loop has a trip count that is uniform over the wave (row slices, chunks, tiles); bounds are lane masks inside them.
#include "gwbp_dev.h"

namespace gwbp {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- means ----------------------------------------------------------------------------------------------------------------------
constexpr int kMeanCols = 64;      // columns per workgroup: one wave reads 256 contiguous bytes of a row
constexpr int kMeanRowLanes = 4;   // waves per workgroup, wave w takes rows w, w + 4, ... of the slice
constexpr int kMeanMaxSlices = 1024;
constexpr int kMeanMinRows = 64;   // rows per slice at least

struct MeanPlan {
    int slices;
    int64_t rows;
};
MeanPlan mean_plan(int64_t N)
{
    int64_t rows = (N + kMeanMaxSlices - 1) / kMeanMaxSlices;
    if (rows < kMeanMinRows)
        rows = kMeanMinRows;
    return {(int)((N + rows - 1) / rows), rows};
}

// MT (the three passes over X): the element type of X, widened as it is loaded (exact); everything else is what it was
template <int MT>
__global__ __launch_bounds__(kMeanCols *kMeanRowLanes) void k_column_sums(int64_t N, int D,
                                                                          const typename MapElem<MT>::raw *__restrict__ X,
                                                                          int64_t ldx, int64_t rows_per_slice,
                                                                          double *__restrict__ partial)
{
    __shared__ double red[kMeanRowLanes][kMeanCols];
    const int cl = threadIdx.x & (kMeanCols - 1), rl = threadIdx.x / kMeanCols; // rl = the wave: its loops are wave-uniform
    const int c = (int)blockIdx.x * kMeanCols + cl;
    const bool on = c < D;
    const int64_t g0 = (int64_t)blockIdx.y * rows_per_slice;
    const int64_t g1 = g0 + rows_per_slice < N ? g0 + rows_per_slice : N;
    typedef MapElem<MT> E;
    const typename E::raw *col = X + (on ? c : 0);
    double acc = 0.0;
    int64_t g = g0 + rl;
    for (; g + 3 * kMeanRowLanes < g1; g += 4 * kMeanRowLanes) { // four rows in flight per thread
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            v[i] = on ? E::cvt(col[(g + i * kMeanRowLanes) * ldx]) : 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            acc += (double)v[i];
    }
    for (; g < g1; g += kMeanRowLanes)
        acc += on ? (double)E::cvt(col[g * ldx]) : 0.0;
    red[rl][cl] = acc;
    __syncthreads();
    if (rl == 0 && on)
        partial[(int64_t)blockIdx.y * D + c] = (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
}

__global__ __launch_bounds__(256) void k_column_means(int64_t N, int D, int slices, const double *__restrict__ partial,
                                                      float *__restrict__ mean)
{
    const int c = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (c >= D)
        return;
    double s = 0.0;
    for (int i = 0; i < slices; ++i)
        s += partial[(int64_t)i * D + c];
    mean[c] = (float)(s / (double)N);
}

// ---- centred Gram ---------------------------------------------------------------------------------------------------------------
constexpr int kGramThreads = 256;            // 4 waves, 2 x 2; each owns a 64 x 64 block of the 128 x 128 output tile
constexpr int kGramT = 128;                  // columns of X per tile side
constexpr int kGramKC = 32;                  // rows of X staged per step
constexpr int kGramLd = 2 * kGramT + 16;     // LDS row stride (floats): the operand reads are ds_read_b32 of 16 consecutive columns
                                             // of rows q and q + 1 per half wave -> 272 = 16 (mod 32) puts them on 32 distinct banks
constexpr int kGramStage = kGramKC * kGramLd; // floats of one staging buffer: [row][tile-row columns | tile-column columns]
constexpr int kGramTargetWgs = 512;          // two workgroups per CU (70 KB of LDS each) on 256 CUs

struct GramPlan {
    int n_tb, n_tiles, slices;
    int64_t rows;
};
// (N, D) alone decide the slices -- and with them every bit of the result
GramPlan gram_plan(int64_t N, int D)
{
    GramPlan p;
    p.n_tb = (D + kGramT - 1) / kGramT;
    p.n_tiles = p.n_tb * (p.n_tb + 1) / 2;
    int want = kGramTargetWgs / p.n_tiles;
    if (want < 1)
        want = 1;
    int64_t rows = (N + want - 1) / want;
    rows = (rows + kGramKC - 1) / kGramKC * kGramKC;
    p.rows = rows;
    p.slices = (int)((N + rows - 1) / rows);
    return p;
}

template <int MT, bool VEC>
__global__ __launch_bounds__(kGramThreads) void k_centered_gram(int64_t N, int D, const typename MapElem<MT>::raw *__restrict__ X,
                                                                int64_t ldx, const float *__restrict__ mean, int64_t rows_per_slice,
                                                                int n_tb, float *__restrict__ partial)
{
    extern __shared__ __attribute__((aligned(16))) float smem[]; // [2][kGramKC][kGramLd]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wa = wave >> 1, wb = wave & 1;
    const int m = lane & 15, qd = lane >> 4;

    // tile (ti <= tj) of the upper triangle, row-major
    int t = (int)blockIdx.x, ti = 0;
    while (t >= n_tb - ti) {
        t -= n_tb - ti;
        ++ti;
    }
    const int tj = ti + t;
    const bool diag = ti == tj;          // one staged block is both operands
    const bool idle = diag && wa > wb;   // the 64 x 64 block below the diagonal: its mirror image is computed by wave (0, 1)

    const int64_t g0 = (int64_t)blockIdx.y * rows_per_slice;
    const int64_t g1 = g0 + rows_per_slice < N ? g0 + rows_per_slice : N;
    const int n_it = (int)((g1 - g0 + kGramKC - 1) / kGramKC);

    // staging role: float4 column c4 of rows r0 + 8 i (i < 4) of the chunk, for the tile's row block and its column block
    const int c4 = (tid & 31) * 4, r0 = tid >> 5;
    const int ca = ti * kGramT + c4, cb = tj * kGramT + c4;
    const float4 ma = load4<false>(mean, ca, D), mb = load4<false>(mean, cb, D); // 0 beyond D, like the columns themselves

    typename MapElem<MT>::raw4 pa[4], pb[4]; // (the bits as loaded: widened where the staging writes them)
    int live = 0; // bit i: row r0 + 8 i of the prefetched chunk exists
    auto prefetch = [&](int it) {
        live = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t g = g0 + (int64_t)it * kGramKC + r0 + 8 * i;
            const typename MapElem<MT>::raw *row = g < g1 ? X + g * ldx : nullptr;
            live |= (row ? 1 : 0) << i;
            pa[i] = load4raw<MT, VEC>(row, ca, D);
            if (!diag)
                pb[i] = load4raw<MT, VEC>(row, cb, D);
        }
    };
    auto centred = [](float4 v, float4 mu, bool on) {
        return on ? make_float4(v.x - mu.x, v.y - mu.y, v.z - mu.z, v.w - mu.w) : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    prefetch(0);

    f32x4 acc[4][4]; // [a][b]: lane holds G[row block column 64 wa + 16 a + 4 qd + r][column block column 64 wb + 16 b + m]
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
            acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int it = 0; it < n_it; ++it) {
        float *buf = smem + (it & 1) * kGramStage;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool on = (live >> i) & 1;
            *reinterpret_cast<float4 *>(buf + (r0 + 8 * i) * kGramLd + c4) = centred(widen4<MT>(pa[i]), ma, on);
            if (!diag)
                *reinterpret_cast<float4 *>(buf + (r0 + 8 * i) * kGramLd + kGramT + c4) = centred(widen4<MT>(pb[i]), mb, on);
        }
        __syncthreads(); // (the buffer written here was last read two steps ago, before the previous barrier)
        if (it + 1 < n_it)
            prefetch(it + 1); // in flight beside this chunk's MFMAs

        if (!idle) {
            const float *oa = buf + qd * kGramLd + wa * 64 + m;
            const float *ob = buf + qd * kGramLd + (diag ? 0 : kGramT) + wb * 64 + m;
#pragma unroll
            for (int s = 0; s < kGramKC / 4; ++s) { // rows 4 s + qd of the chunk: the four k slots of one MFMA
                float fa[4], fb[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    fa[a] = oa[4 * s * kGramLd + 16 * a];
                    fb[a] = ob[4 * s * kGramLd + 16 * a];
                }
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[a], fb[b], acc[a][b], 0, 0, 0);
            }
        }
    }

    if (idle)
        return;
    float *out = partial + (int64_t)blockIdx.y * D * D;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int col = tj * kGramT + wb * 64 + 16 * b + m;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = ti * kGramT + wa * 64 + 16 * a + 4 * qd + r;
                if (row < D && col < D)
                    out[(int64_t)row * D + col] = acc[a][b][r];
            }
        }
}

// G[a, b] = sum over the slices, ascending, in float64, of the partial entry at (min(a, b), max(a, b)): every entry with a <= b
// lies in a tile of the upper triangle and in a 64 x 64 block on or above the diagonal, the only ones k_centered_gram writes.
__global__ __launch_bounds__(256) void k_gram_reduce(int D, int slices, const float *__restrict__ partial, double *__restrict__ G)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)D * D)
        return;
    const int a = (int)(e / D), b = (int)(e % D);
    const int64_t at = a <= b ? e : (int64_t)b * D + a;
    double s = 0.0;
    for (int i = 0; i < slices; ++i)
        s += (double)partial[(int64_t)i * D * D + at];
    G[e] = s;
}

// ---- projection -----------------------------------------------------------------------------------------------------------------
constexpr int kProjThreads = 256;  // 4 waves, each owns 32 of the workgroup's rows
constexpr int kProjRows = GWBP_PCA_PROJECT_ROWS;
constexpr int kProjKC = 32;        // columns staged per step
constexpr int kProjLd = kProjKC + 4;
constexpr int kProjMaxK = 16;
static_assert(kProjRows == 128, "four waves x two 16-row MFMA blocks");

template <int MT, bool VEC>
__global__ __launch_bounds__(kProjThreads) void k_pca_project(int64_t N, int D, int k,
                                                              const typename MapElem<MT>::raw *__restrict__ X, int64_t ldx,
                                                              const float *__restrict__ mean, const float *__restrict__ V,
                                                              float *__restrict__ Y, float *__restrict__ minmax)
{
    __shared__ __attribute__((aligned(16))) float sx[2][kProjRows * kProjLd];
    __shared__ __attribute__((aligned(16))) float sv[2][kProjMaxK * kProjLd];
    __shared__ float red[2][4];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = lane & 15, qd = lane >> 4;
    const int64_t q0 = (int64_t)blockIdx.x * kProjRows;

    // staging role: float4 column c4 of rows r0 + 32 i (i < 4) of X, and (threads 0..127) of component r0
    const int c4 = (tid & 7) * 4, r0 = tid >> 3;
    const typename MapElem<MT>::raw *xrow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t g = q0 + r0 + 32 * i;
        xrow[i] = g < N ? X + g * ldx : nullptr;
    }
    const float *vrow = (tid < kProjMaxK * 8 && r0 < k) ? V + (int64_t)r0 * D : nullptr;

    const int n_chunk = (D + kProjKC - 1) / kProjKC;
    typename MapElem<MT>::raw4 px[4];
    float4 pv, pm;
    auto prefetch = [&](int chunk) {
        const int c = chunk * kProjKC + c4;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            px[i] = load4raw<MT, VEC>(xrow[i], c, D);
        pv = load4<false>(vrow, c, D);
        pm = load4<false>(mean, c, D);
    };
    prefetch(0);

    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}}; // [rb]: row 32 wave + 16 rb + m, components 4 qd + r
    for (int chunk = 0; chunk < n_chunk; ++chunk) {
        float *bx = sx[chunk & 1], *bv = sv[chunk & 1];
#pragma unroll
        for (int i = 0; i < 4; ++i) { // (a row beyond N stages -mu: its Y is never written or counted)
            const float4 x = widen4<MT>(px[i]);
            *reinterpret_cast<float4 *>(bx + (r0 + 32 * i) * kProjLd + c4) = make_float4(x.x - pm.x, x.y - pm.y, x.z - pm.z, x.w - pm.w);
        }
        if (tid < kProjMaxK * 8)
            *reinterpret_cast<float4 *>(bv + r0 * kProjLd + c4) = pv;
        __syncthreads();
        if (chunk + 1 < n_chunk)
            prefetch(chunk + 1);

        const float *ox = bx + (wave * 32 + m) * kProjLd + 4 * qd;
        const float *ov = bv + m * kProjLd + 4 * qd;
#pragma unroll
        for (int kb = 0; kb < kProjKC / 16; ++kb) {
            const float4 fv = *reinterpret_cast<const float4 *>(ov + kb * 16);
            float4 fx[2];
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
                fx[rb] = *reinterpret_cast<const float4 *>(ox + rb * 16 * kProjLd + kb * 16);
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
                acc[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(fv.x, fx[rb].x, acc[rb], 0, 0, 0);
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
                acc[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(fv.y, fx[rb].y, acc[rb], 0, 0, 0);
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
                acc[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(fv.z, fx[rb].z, acc[rb], 0, 0, 0);
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
                acc[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(fv.w, fx[rb].w, acc[rb], 0, 0, 0);
        }
    }

    // min and max are exact: the smallest / largest of the partials is Y's, bit for bit (a NaN entry is skipped: fit first)
    float lo = __builtin_inff(), hi = -__builtin_inff();
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        const int64_t g = q0 + wave * 32 + 16 * rb + m;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = 4 * qd + r;
            if (g < N && j < k) {
                const float y = acc[rb][r];
                Y[g * k + j] = y;
                lo = fminf(lo, y);
                hi = fmaxf(hi, y);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    if (lane == 0) {
        red[0][wave] = lo;
        red[1][wave] = hi;
    }
    __syncthreads();
    if (tid == 0) { // (wave 0 always holds an existing row, so neither value is left infinite)
        minmax[2 * (int64_t)blockIdx.x] = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
        minmax[2 * (int64_t)blockIdx.x + 1] = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
    }
}

// colors = (Y - lo) / (hi - lo), one lo and hi for every channel (visualize_pca.py's np.min / np.max over all of them); a field
// without spread (hi == lo) gets 0.5 everywhere instead of 0 / 0.
__global__ __launch_bounds__(256) void k_pca_colors(int64_t n, const float *__restrict__ Y, const float *__restrict__ lo_hi,
                                                    float *__restrict__ out)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n)
        return;
    const float lo = lo_hi[0], span = lo_hi[1] - lo;
    out[e] = span > 0.f ? (Y[e] - lo) / span : 0.5f;
}

} // namespace

size_t pca_workspace_bytes(int64_t N, int D)
{
    const size_t means = (size_t)mean_plan(N).slices * D * sizeof(double);
    const size_t gram = (size_t)gram_plan(N, D).slices * D * D * sizeof(float);
    return means > gram ? means : gram;
}

int launch_column_means(int64_t N, int D, const void *X, int mt, int64_t ldx, float *mean, void *ws, hipStream_t s)
{
    const MeanPlan p = mean_plan(N);
    double *partial = static_cast<double *>(ws);
    const dim3 grid((unsigned)((D + kMeanCols - 1) / kMeanCols), (unsigned)p.slices);
    with_map_type(mt, [&](auto MT) {
        hipLaunchKernelGGL(k_column_sums<MT>, grid, dim3(kMeanCols * kMeanRowLanes), 0, s, N, D, field_ptr<MT>(X), ldx, p.rows, partial);
    });
    hipLaunchKernelGGL(k_column_means, dim3((unsigned)((D + 255) / 256)), dim3(256), 0, s, N, D, p.slices, partial, mean);
    return check_hip(hipGetLastError(), "column_means launch");
}

int launch_centered_gram(int64_t N, int D, const void *X, int mt, int64_t ldx, const float *mean, double *gram, void *ws,
                         hipStream_t s)
{
    const GramPlan p = gram_plan(N, D);
    float *partial = static_cast<float *>(ws);
    const int lds = 2 * kGramStage * (int)sizeof(float);
    const dim3 grid((unsigned)p.n_tiles, (unsigned)p.slices);
    const int rc = with_field_type(mt, field_rows_vec(X, ldx, mt), [&](auto MT, auto VEC) {
        if (int e = ensure_dynamic_lds(reinterpret_cast<const void *>(k_centered_gram<MT, VEC>), lds))
            return e;
        hipLaunchKernelGGL((k_centered_gram<MT, VEC>), grid, dim3(kGramThreads), lds, s, N, D, field_ptr<MT>(X), ldx, mean, p.rows,
                           p.n_tb, partial);
        return (int)GWBP_OK;
    });
    if (rc)
        return rc;
    hipLaunchKernelGGL(k_gram_reduce, dim3((unsigned)(((int64_t)D * D + 255) / 256)), dim3(256), 0, s, D, p.slices, partial, gram);
    return check_hip(hipGetLastError(), "centered_gram launch");
}

int launch_pca_project(int64_t N, int D, int k, const void *X, int mt, int64_t ldx, const float *mean, const float *V, float *Y,
                       float *minmax, hipStream_t s)
{
    unsigned grid = 0;
    if (int rc = grid_of("pca_project", N, &grid, kProjRows))
        return rc;
    with_field_type(mt, field_rows_vec(X, ldx, mt), [&](auto MT, auto VEC) {
        hipLaunchKernelGGL((k_pca_project<MT, VEC>), dim3(grid), dim3(kProjThreads), 0, s, N, D, k, field_ptr<MT>(X), ldx, mean, V, Y,
                           minmax);
    });
    return check_hip(hipGetLastError(), "pca_project launch");
}

int launch_pca_colors(int64_t n, const float *Y, const float *lo_hi, float *colors, hipStream_t s)
{
    if (n == 0)
        return GWBP_OK;
    unsigned grid = 0;
    if (int rc = grid_of("pca_colors", n, &grid, 256))
        return rc;
    hipLaunchKernelGGL(k_pca_colors, dim3(grid), dim3(256), 0, s, n, Y, lo_hi, colors);
    return check_hip(hipGetLastError(), "pca_colors launch");
}

} // namespace gwbp
