// field_compare_kernel.h -- k_field_compare as a template over the element types of the field (FT) and of the map (MT), and its typed
// launcher: field_compare.hip instantiates it for fp32 fields, field_compare_half.hip for fp16 / bf16 ones.  k_field_compare: a D-wide field rendered from the weight store and compared, inside the kernel, with the
// 2-D map of the view it was lifted from.  Per pixel p, with r(p) = sum_g w_g(p) F[g, :] (gwbp_render's values bit for bit) and
// m(p, :) the map row, five fp32 sums over the channels leave the kernel instead of the [H, W, D] image:
//   dot = sum r m     rr = sum r r     mm = sum m m     l1 = sum |r - m|     l2 = sum (r - m)^2
// and a sixth plane derived from them, cosine = dot / sqrt(rr mm) (float64 arithmetic, one rounding to fp32; NaN where rr mm = 0).
//
// The walk is k_render_rows4's (render_wide.hip): a wave owns ONE ROW of a tile (16 pixels), lanes = channel quads, the 16
// accumulators are registers, the row's records are found by a vote over 64 headers and walked through a software pipeline of
// SLOTS visits.  Every pixel is summed front to back by fmaf(w, F[g, c], acc) in record order -- the order of gwbp_render for
// every D, because a pixel's chain does not depend on which lane holds the channel.  So ONE walk serves every D here: rows that
// are not 16-B aligned or D % 4 != 0 (k_render_rows' territory in gwbp_render) take the same lane layout with element loads.
// The chunks of a wide field are walked by the SAME wave one after the other (a tile row has no second owner, so nothing has to be
// combined between waves, and 16 rows x thousands of tiles are waves enough without the chunks): 512 channels per walk while
// whole blocks of 512 remain and the rows are aligned, 256 otherwise.
//
// REDUCTION ORDER (depends on D alone, not on alignment, map type or the walk's width):
//   block b    = channels 256 b .. 256 b + 255; lane l holds channels 256 b + 4 l + k, k = 0..3
//   lane term  = a chain over k = 0, 1, 2, 3 from +0: fmaf for dot, rr, mm and l2, a plain add of |r - m| for l1
//   block sum  = wave_sum (gwbp_dev.h) of the 64 lane terms: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror,
//                then (row 0 + row 1) + (row 2 + row 3); lanes past D hold +0
//   pixel sum  = the block sums added in ascending b, from +0
// Per-view sums: float64, per tile row over its 16 pixels by xor-butterfly (8, 4, 2, 1; operands commute, every lane gets the same
// bits), the rows by k_compare_table: thread t adds rows t, t + 1024, ... ascending, then a halving tree over the 1024 threads.
// No atomics anywhere; every loop is wave-uniform with a bound known at launch; every store is an ordinary vector store.
//
// A map row with a non-finite element makes the pixel BAD: NaN in all six planes, counted in n_bad, left out of the sums.  A pixel
// is VALID when it is not bad, its five sums are finite, rr > 0 and mm > 0; the sums of the table run over the valid pixels.
//
// A half FIELD (FT = fp16 / bf16, row stride in elements) is read as stored: a visit's slot holds the bits its loads landed (four
// halves in a uint2 per quad, k_render_rows4's raw slots; four zero-extended elements on the element path) and process() widens them
// (exact) behind the step's loads.  The FMAs see the widened values in the same order: the bits of the fp32 kernel on features.float().
#pragma once
#include "gwbp_dev.h"

namespace gwbp {

namespace {

constexpr int kSlots1 = 4; // visits in flight at 256 channels per walk, as GWBP_RENDER_SLOTS
constexpr int kSlots2 = 3; // ... and at 512, as GWBP_RENDER_SLOTS2
constexpr int kRowSums = 6; // per tile row: sum cosine, sum l1, sum l2, sum mm, n_valid, n_bad (float64)

struct CmpMap { // the view's map as the epilogue addresses it; strides in elements, unit channel stride
    const void *p;
    int64_t sy, sx;
    const int32_t *ymap, *xmap; // row / column of a low-resolution [lr_h, lr_w, D] map per output row / column, or nullptr
    int lr_h, lr_w;
};

struct Desc { // wave-uniform
    u32 gid, off, bits;
    bool have;
};

__device__ __forceinline__ float readlane_f(float v, int l)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

__device__ __forceinline__ bool nonfinite(float x) { return (__float_as_uint(x) & 0x7F800000u) == 0x7F800000u; }

// Four channels of one row of the field from channel c on, as LOADED (field4) and as values (widen).  VEC: one 16-B load of an fp32
// row, one 8-B load of a half row (the caller keeps c inside the row); otherwise element loads whose indices are clamped into the row
// (what lies past D is masked by the caller), four zero-extended elements of a half row.
template <int FT, bool VEC>
struct Quad {
    typedef typename MapElem<FT>::raw raw;
    typedef std::conditional_t<FT == GWBP_MAP_F32, float4, std::conditional_t<VEC, uint2, uint4>> type;
    static __device__ __forceinline__ type field4(const raw *__restrict__ row, int c, int D)
    {
        if constexpr (VEC)
            return *reinterpret_cast<const type *>(row + c);
        else if constexpr (FT == GWBP_MAP_F32)
            return make_float4(row[min(c, D - 1)], row[min(c + 1, D - 1)], row[min(c + 2, D - 1)], row[min(c + 3, D - 1)]);
        else
            return make_uint4(row[min(c, D - 1)], row[min(c + 1, D - 1)], row[min(c + 2, D - 1)], row[min(c + 3, D - 1)]);
    }
    static __device__ __forceinline__ float4 widen(type r)
    {
        typedef MapElem<FT> E;
        if constexpr (FT == GWBP_MAP_F32)
            return r;
        else if constexpr (VEC)
            return E::cvt4(r);
        else
            return make_float4(E::cvt((unsigned short)r.x), E::cvt((unsigned short)r.y), E::cvt((unsigned short)r.z),
                               E::cvt((unsigned short)r.w));
    }
};

template <int MT, bool VEC>
__device__ __forceinline__ float4 map4(const void *__restrict__ row, int c, int D)
{
    typedef MapElem<MT> E;
    if (VEC)
        return E::cvt4(*reinterpret_cast<const typename E::raw4 *>(static_cast<const typename E::raw *>(row) + c));
    const typename E::raw *r = static_cast<const typename E::raw *>(row);
    return make_float4(E::cvt(r[min(c, D - 1)]), E::cvt(r[min(c + 1, D - 1)]), E::cvt(r[min(c + 2, D - 1)]),
                       E::cvt(r[min(c + 3, D - 1)]));
}

// k_render_rows4's walk for the 256 * Q channels from cb on (cb < D): acc[p][j] = the render of pixel p of the wave's tile row at
// channels cb + 256 j + 4 lane + 0..3.  Lanes whose quad starts past D re-read a valid address; what they hold is masked later.
template <int FT, int Q, int SLOTS, bool VEC>
__device__ __forceinline__ void walk_row(float4 (&acc)[16][Q], u32 nh, const Header *__restrict__ hbase, int q, u32 sh,
                                         const WPair *__restrict__ wpool, const typename MapElem<FT>::raw *__restrict__ feats,
                                         int64_t ldf, int D, int cb, int lane)
{
    typedef Quad<FT, VEC> Q4;
    struct Data4 {
        float w;
        typename Q4::type col[Q]; // as loaded
    };
    int c0[Q];
#pragma unroll
    for (int j = 0; j < Q; ++j) {
        const int c = cb + 256 * j + 4 * lane;
        c0[j] = c < D ? c : cb;
    }
#pragma unroll
    for (int p = 0; p < 16; ++p)
#pragma unroll
        for (int j = 0; j < Q; ++j)
            acc[p][j] = make_float4(0.f, 0.f, 0.f, 0.f);

    for (u32 h0 = 0; h0 < nh; h0 += 64) {
        const u32 hh = min(h0 + (u32)lane, nh - 1);
        const Header *hp = hbase + hh;
        const u64 m = (h0 + (u32)lane < nh) ? hp->mask[q] : 0ull;
        const u32 my_bits = (u32)(m >> sh) & 0xFFFFu;
        const u32 my_gid = hp->gid;
        const u32 my_off = hp->woff[q] + (u32)__popcll(m & ((1ull << sh) - 1ull));
        u64 rem = __ballot(my_bits != 0u);
        if (rem == 0ull)
            continue;

        Desc ds[SLOTS];
        Data4 dt[SLOTS];
        auto refill = [&](Desc &d_, Data4 &x_) __attribute__((always_inline)) {
            u32 gid_s = d_.gid, off_s = d_.off, bits_s = 0u; // exhausted: re-read the slot's last (valid) addresses
            d_.have = rem != 0ull;
            if (d_.have) {
                const int l = __ffsll((long long)rem) - 1;
                rem &= rem - 1ull;
                gid_s = (u32)__builtin_amdgcn_readlane((int)my_gid, l);
                off_s = (u32)__builtin_amdgcn_readlane((int)my_off, l);
                bits_s = (u32)__builtin_amdgcn_readlane((int)my_bits, l);
            }
            d_.gid = gid_s, d_.off = off_s, d_.bits = bits_s;
            // lane k < 16 reads entry k of the visit; lanes past its last entry read the next records' entries or the slack behind
            // the pool (make_layout) and are never looked at (v_readlane k < count)
            x_.w = wpool[off_s + (u32)(lane & 15)].w;
#pragma unroll
            for (int j = 0; j < Q; ++j)
                x_.col[j] = Q4::field4(feats + (int64_t)gid_s * ldf, c0[j], D);
        };
        auto process = [&](const Desc &d_, const Data4 &x_) __attribute__((always_inline)) {
            if (!d_.have)
                return;
            float4 cv[Q]; // widened here, behind the step's loads (the identity for an fp32 field)
#pragma unroll
            for (int j = 0; j < Q; ++j)
                cv[j] = Q4::widen(x_.col[j]);
            int k = 0;
#pragma unroll
            for (int p = 0; p < 16; ++p) {
                if ((d_.bits >> p) & 1u) { // wave-uniform
                    const float w = readlane_f(x_.w, k);
                    ++k;
#pragma unroll
                    for (int j = 0; j < Q; ++j) {
                        acc[p][j].x = __builtin_fmaf(w, cv[j].x, acc[p][j].x);
                        acc[p][j].y = __builtin_fmaf(w, cv[j].y, acc[p][j].y);
                        acc[p][j].z = __builtin_fmaf(w, cv[j].z, acc[p][j].z);
                        acc[p][j].w = __builtin_fmaf(w, cv[j].w, acc[p][j].w);
                    }
                }
            }
        };
        // the first touched record gives every slot a valid address before any refill may run dry
        {
            const int l0 = __ffsll((long long)rem) - 1;
            const u32 g0 = (u32)__builtin_amdgcn_readlane((int)my_gid, l0);
            const u32 o0 = (u32)__builtin_amdgcn_readlane((int)my_off, l0);
#pragma unroll
            for (int s = 0; s < SLOTS; ++s)
                ds[s].gid = g0, ds[s].off = o0, ds[s].bits = 0u, ds[s].have = false;
        }
#pragma unroll
        for (int s = 0; s < SLOTS; ++s)
            refill(ds[s], dt[s]);
        while (ds[0].have) { // slots fill in order, so slot 0 runs dry first only when everything has: at most 64 / SLOTS + 1 rounds
#pragma unroll
            for (int s = 0; s < SLOTS; ++s) {
                process(ds[s], dt[s]);
                refill(ds[s], dt[s]);
            }
        }
    }
}

struct RowState {  // of the wave's 16 pixels
    float s[5];    // lane p < 16: pixel p's dot, rr, mm, l1, l2 so far
    u32 bad;       // wave-uniform: bit p = pixel p's map row holds a non-finite element
    int yy, xv;    // wave-uniform map row; lane p < 16: pixel p's map column
};

// The compare epilogue of one walk: the 16 pixels' map rows at the walk's channels against acc, block by block.
template <int MT, int Q, bool VEC>
__device__ __forceinline__ void compare_chunk(const float4 (&acc)[16][Q], const CmpMap &M, int D, int cb, int lane, int n_px,
                                              RowState &R)
{
    typedef typename MapElem<MT>::raw raw;
    const raw *base = static_cast<const raw *>(M.p) + (int64_t)R.yy * M.sy;
#pragma unroll
    for (int p = 0; p < 16; ++p) {
        if (p >= n_px) // wave-uniform: a pixel of a partial edge tile outside the image is neither read nor written
            continue;
        const int xx = __builtin_amdgcn_readlane(R.xv, p);
        const raw *row = base + (int64_t)xx * M.sx;
#pragma unroll
        for (int j = 0; j < Q; ++j) {
            const int c = cb + 256 * j + 4 * lane;
            if (cb + 256 * j >= D) // wave-uniform: the walk's second block lies past the field
                continue;
            const float4 mv = map4<MT, VEC>(row, c < D ? c : cb, D);
            const float4 rv = acc[p][j];
            const float m[4] = {mv.x, mv.y, mv.z, mv.w}, r[4] = {rv.x, rv.y, rv.z, rv.w};
            float t[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
            bool nf = false;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool on = c + k < D;
                const float mk = on ? m[k] : 0.f, rk = on ? r[k] : 0.f;
                nf = nf || (on && nonfinite(m[k]));
                const float df = rk - mk;
                t[0] = __builtin_fmaf(rk, mk, t[0]);
                t[1] = __builtin_fmaf(rk, rk, t[1]);
                t[2] = __builtin_fmaf(mk, mk, t[2]);
                t[3] = t[3] + __builtin_fabsf(df);
                t[4] = __builtin_fmaf(df, df, t[4]);
            }
            if (__ballot(nf) != 0ull)
                R.bad |= 1u << p;
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const float tot = wave_sum(t[i]);
                R.s[i] = lane == p ? R.s[i] + tot : R.s[i];
            }
        }
    }
}

__device__ __forceinline__ double butterfly16(double v)
{
    v += __shfl_xor(v, 8);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 1);
    return v;
}

// WIDE2: whole blocks of 512 channels are walked 512 at a time (needs VEC).  empty: the scene has no Gaussian (nothing of the
// store is read).  planes: [6][H][W] or nullptr.  rowsums: [tiles][16][kRowSums] float64.
template <int FT, int MT, bool WIDE2, bool VEC>
__global__ __launch_bounds__(256) void k_field_compare(ViewDev V, int empty, const u32 *__restrict__ tile_offsets,
                                                       const u32 *__restrict__ hdr_count, const Header *__restrict__ headers,
                                                       const WPair *__restrict__ wpool,
                                                       const typename MapElem<FT>::raw *__restrict__ feats, int64_t ldf, int D,
                                                       CmpMap M, float *__restrict__ planes, double *__restrict__ rowsums)
{
    // blockIdx -> (tile, quarter) as in k_render_rows: the four blocks of a tile share an XCD
    const u32 b = blockIdx.x;
    const u32 x = b & 7u, sidx = b >> 3;
    const int tile = (int)((sidx >> 2) * 8u + x);
    if (tile >= V.tile_w * V.tile_h)
        return;
    const int q = (int)(sidx & 3u);
    const int lane = threadIdx.x & 63;
    const int wave = (int)uniform(threadIdx.x >> 6);
    const int tx = tile % V.tile_w, ty = tile / V.tile_w;
    const int iy = ty * kTile + 4 * q + wave;
    if (iy >= V.H)
        return; // whole wave; no barriers in this kernel
    const u32 sh = 16u * (u32)wave;
    const int x0 = tx * kTile;
    const int n_px = min(kTile, V.W - x0);
    const u32 nh = empty ? 0u : uniform(hdr_count[tile]);
    const Header *hbase = headers + (empty ? 0u : uniform(tile_offsets[tile]));

    RowState R;
#pragma unroll
    for (int i = 0; i < 5; ++i)
        R.s[i] = 0.f;
    R.bad = 0u;
    {
        // the index maps are clamped into the map: a stray index reads a wrong texel, never memory outside the map
        int yy = iy, xv = min(x0 + (lane & 15), V.W - 1);
        if (M.ymap)
            yy = min(max((int)uniform((u32)M.ymap[iy]), 0), M.lr_h - 1);
        if (M.xmap)
            xv = min(max(M.xmap[xv], 0), M.lr_w - 1);
        R.yy = yy, R.xv = xv;
    }

    int cb = 0;
    if constexpr (WIDE2) {
        const int n8 = D / 512; // <= GWBP_PCA_MAX_D / 512
        for (int i = 0; i < n8; ++i, cb += 512) {
            float4 acc[16][2];
            walk_row<FT, 2, kSlots2, VEC>(acc, nh, hbase, q, sh, wpool, feats, ldf, D, cb, lane);
            compare_chunk<MT, 2, VEC>(acc, M, D, cb, lane, n_px, R);
        }
    }
    for (; cb < D; cb += 256) { // <= GWBP_PCA_MAX_D / 256 rounds
        float4 acc[16][1];
        walk_row<FT, 1, kSlots1, VEC>(acc, nh, hbase, q, sh, wpool, feats, ldf, D, cb, lane);
        compare_chunk<MT, 1, VEC>(acc, M, D, cb, lane, n_px, R);
    }

    // ---- lane p < n_px: pixel p's planes and its share of the row's sums ------------------------------------------------------
    const bool mine = lane < n_px;
    const bool bad = mine && ((R.bad >> (lane & 15)) & 1u);
    const float nanf = __uint_as_float(0x7FC00000u);
    float dot = R.s[0], rr = R.s[1], mm = R.s[2], l1 = R.s[3], l2 = R.s[4];
    const double rrmm = (double)rr * (double)mm; // exact: never 0 unless a factor is
    float cosv = rrmm > 0.0 ? (float)((double)dot / __builtin_sqrt(rrmm)) : nanf;
    if (bad)
        dot = rr = mm = l1 = l2 = cosv = nanf;
    const bool valid = mine && !bad && rr > 0.f && mm > 0.f &&
                       !(nonfinite(dot) || nonfinite(rr) || nonfinite(mm) || nonfinite(l1) || nonfinite(l2));
    if (planes && mine) {
        const size_t hw = (size_t)V.H * (size_t)V.W, at = (size_t)iy * (size_t)V.W + (size_t)(x0 + lane);
        planes[at] = dot;
        planes[hw + at] = rr;
        planes[2 * hw + at] = mm;
        planes[3 * hw + at] = l1;
        planes[4 * hw + at] = l2;
        planes[5 * hw + at] = cosv;
    }
    const double s_cos = butterfly16(valid ? (double)cosv : 0.0), s_l1 = butterfly16(valid ? (double)l1 : 0.0);
    const double s_l2 = butterfly16(valid ? (double)l2 : 0.0), s_mm = butterfly16(valid ? (double)mm : 0.0);
    const u64 v_mask = __ballot(valid), b_mask = __ballot(bad);
    if (lane == 0) {
        double *o = rowsums + ((size_t)tile * 16u + (size_t)(4 * q + wave)) * kRowSums;
        o[0] = s_cos, o[1] = s_l1, o[2] = s_l2, o[3] = s_mm;
        o[4] = (double)__popcll(v_mask), o[5] = (double)__popcll(b_mask);
    }
}

template <int FT, int MT>
void launch_compare_mt(bool wide2, bool vec, unsigned grid, hipStream_t s, const ViewDev &V, int empty, const Ws &W,
                       const void *feats_v, int64_t ldf, int D, const CmpMap &M, float *planes, double *rowsums)
{
    const auto *feats = field_ptr<FT>(feats_v);
#define GWBP_CMP(W2, VC)                                                                                                             \
    hipLaunchKernelGGL((k_field_compare<FT, MT, W2, VC>), dim3(grid), dim3(256), 0, s, V, empty, W.tile_offsets, W.hdr_count, W.headers, \
                       W.wpool, feats, ldf, D, M, planes, rowsums)
    if (wide2)
        GWBP_CMP(true, true);
    else if (vec)
        GWBP_CMP(false, true);
    else
        GWBP_CMP(false, false);
#undef GWBP_CMP
}

// every map type for one field type; the caller checks the launch
template <int FT>
void launch_compare_ft(int mt, bool wide2, bool vec, unsigned grid, hipStream_t s, const ViewDev &V, int empty, const Ws &W,
                       const void *feats, int64_t ldf, int D, const CmpMap &M, float *planes, double *rowsums)
{
    with_map_type(mt, [&](auto MT) { launch_compare_mt<FT, MT>(wide2, vec, grid, s, V, empty, W, feats, ldf, D, M, planes, rowsums); });
}

} // namespace

} // namespace gwbp
