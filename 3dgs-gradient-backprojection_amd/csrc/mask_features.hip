// mask_features.hip -- back-projection of MASK-POOLED features: a label map L [H, W] (a segmenter's masks or instances,
// superpixels) and one embedding per label, table E [M, D] (a CLIP / LSeg vector per mask):
//     F[g, :] += scale_f * sum_p w_g(p) E[L(p), :],     d[g] += scale_d * sum_p w_g(p)
// = gwbp_scatter on the materialised map E[L] (a zero row where L(p) is outside [0, M)) without the [H, W, D] map and without
// the dense scatter's flush atomics.  See mask_features.h for the formulation.
//
// k_zero_mask_sums: the sums of this view's n_isect emit positions are cleared (an emit position without a record -- no pixel of
//   the tile had weight -- must read as empty).
// k_mask_reduce: one workgroup per tile (heaviest first), four waves, one (Gaussian, tile) record per wave at a time -- the reduce
//   by key of k_scatter_labels (label.hip) over the same two dense runs of the weight store.  The tile's labels are staged in LDS
//   (-1 outside [0, M), read through the nearest index maps for a low-resolution map); a leader label is matched by every lane and
//   its weights summed across the wave.  The first kMaskSlots (label, sum) pairs of the record, -1 included (its weight counts in
//   d only), go to the record's emit position estart[gid] + its tile's row-major index in rect[gid] (the arithmetic of
//   k_blend<kToken>).  A record with more distinct labels SPILLS the rest: its further pairs are listed in LDS and the wave adds
//   sum_k s_k E[k, :] to F[gid, :] with D fp32 atomics (and their weight to d with one), and counts the record in *n_spilled.
// k_mask_apply: one wave per Gaussian at a time, 16 consecutive Gaussians of the depth order per wave (the emit order): the
//   Gaussian's slots lie back to back.  Per batch of 16 emit positions x 4 slots (one per lane) the equal labels are merged
//   (leader + wave sum), the table rows of up to kMaskFlight labels are read together (from L2: 0.4 MB at M = 200, D = 512) and
//   multiplied into registers, and F[gid, :] and d[gid] then get ONE plain read-modify-write per view -- no atomics, the order of
//   every sum fixed: without spills F and d are the same bit for bit from run to run.  The NEXT Gaussian's F row, first slots
//   and d are requested before the current one is worked on (k_token_apply's two register sets).  Half tables are widened as
//   they are read (8-B loads of four channels), so F equals that of table.float().
#include "mask_features.h"
#include "token_kernel.h" // f4, load_tok

namespace gwbp {

constexpr int kMaskThreads = 256;  // k_mask_reduce: one workgroup per tile, four waves
constexpr int kMaskEntries = 4;    // a record holds at most 256 entries: four per lane
constexpr int kMaskPerWave = 16;   // k_mask_apply: Gaussians (consecutive in depth order) per wave
constexpr int kMaskWaves = 4;
constexpr int kMaskGroup = kMaskPerWave * kMaskWaves;

__global__ __launch_bounds__(256) void k_zero_mask_sums(float4 *__restrict__ sums, const Counters *__restrict__ ctr)
{
    if (ctr->overflow & 1u)
        return; // (n_isect reads 0 then anyway)
    const u32 n = ctr->n_isect;
    for (u32 i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u)
        sums[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}

template <typename T, int MT>
__global__ __launch_bounds__(kMaskThreads) void k_mask_reduce(
    ViewDev V, const u32 *__restrict__ tile_order, const u32 *__restrict__ tile_offsets, const u32 *__restrict__ hdr_count,
    const Header *__restrict__ headers, const WPair *__restrict__ wpool, const u32 *__restrict__ estart,
    const uint2 *__restrict__ rect, const T *__restrict__ labels, int64_t ls_y, int64_t ls_x, const int32_t *__restrict__ ymap,
    const int32_t *__restrict__ xmap, int M, const void *__restrict__ table_v, int64_t ts_row, int D, float scale_f, float scale_d,
    float *__restrict__ F, float *__restrict__ d, int4 *__restrict__ slot_lab, float4 *__restrict__ slot_sum,
    u32 *__restrict__ n_spilled, Counters *__restrict__ ctr)
{
    typedef typename MapElem<MT>::raw TR;
    const TR *const table = static_cast<const TR *>(table_v);
    const u32 kind = ctr->blend_kind;
    if (kind == kBlendFused || kind == kBlendToken) { // the workspace holds no weight store: refuse, flag
        if (blockIdx.x == 0 && threadIdx.x == 0)
            atomicOr(&ctr->overflow, kOverflowMismatch);
        return;
    }
    if (ctr->overflow & 1u) // an intersection-capacity overflow leaves no emit positions (estart is stale): nothing is filed
        return;
    const u32 n_isect = ctr->n_isect;
    const int tile = (int)tile_order[blockIdx.x];
    const u32 nh = hdr_count[tile];
    if (nh == 0)
        return;
    const int tx = tile % V.tile_w, ty = tile / V.tile_w;

    __shared__ int s_lab[kTilePix];
    {
        const int p = threadIdx.x; // kMaskThreads == kTilePix
        const int ix = tx * kTile + (p & 15), iy = ty * kTile + (p >> 4);
        int lab = -1;
        if (ix < V.W && iy < V.H) {
            const int64_t row = ymap ? ymap[iy] : iy, col = xmap ? xmap[ix] : ix;
            const int v = (int)labels[row * ls_y + col * ls_x];
            lab = (v >= 0 && v < M) ? v : -1;
        }
        s_lab[p] = lab;
    }
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const u32 wave = uniform(threadIdx.x >> 6);
    // a spilled record's pairs beyond the slots (at most 256 distinct labels per record)
    __shared__ int s_key[kMaskThreads / 64][kTilePix];
    __shared__ float s_sum[kMaskThreads / 64][kTilePix];
    const Header *hb = headers + tile_offsets[tile];

    for (u32 h = wave; h < nh; h += kMaskThreads / 64) {
        const Header *hp = hb + h;
        const u32 gid = uniform(hp->gid), w0 = uniform(hp->woff[0]), w2 = uniform(hp->woff[2]);
        const u32 counts = uniform(hp->counts);
        const u32 n01 = (counts & 0xFFu) + ((counts >> 8) & 0xFFu);
        const u32 n = n01 + ((counts >> 16) & 0xFFu) + (counts >> 24);
        const uint2 rc = rect[gid];
        const u32 rx0 = rc.x & 0xFFFFu, rx1 = rc.x >> 16, ry0 = rc.y & 0xFFFFu;
        const u32 pos = uniform(estart[gid] + ((u32)ty - ry0) * (rx1 - rx0) + ((u32)tx - rx0));

        int lab[kMaskEntries];
        float w[kMaskEntries];
        bool pend[kMaskEntries];
#pragma unroll
        for (int k = 0; k < kMaskEntries; ++k) {
            lab[k] = -1, w[k] = 0.f, pend[k] = false;
            const u32 i = (u32)(k * 64 + lane);
            if ((u32)(k * 64) < n && i < n) {
                const WPair e = wpool[i < n01 ? w0 + i : w2 + (i - n01)];
                w[k] = e.w;
                lab[k] = s_lab[e.pix]; // (a stored entry's pixel is < 256; only padding carries kPadPix, and it is not read)
                pend[k] = true;        // -1 included: its weight is filed for d
            }
        }
        int key_s[kMaskSlots];
        float sum_s[kMaskSlots];
#pragma unroll
        for (int j = 0; j < kMaskSlots; ++j)
            key_s[j] = -1, sum_s[j] = 0.f;
        u32 r = 0; // distinct labels of the record so far (wave-uniform)
        float dsp = 0.f;
        for (;;) {
            u64 any = 0ull;
#pragma unroll
            for (int k = 0; k < kMaskEntries; ++k)
                any |= __builtin_amdgcn_ballot_w64(pend[k]);
            if (any == 0ull)
                break;
            int cand = -1; // this lane's first pending label
#pragma unroll
            for (int k = kMaskEntries - 1; k >= 0; --k)
                cand = pend[k] ? lab[k] : cand;
            const int key = __builtin_amdgcn_readlane(cand, (int)__builtin_ctzll(any));
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < kMaskEntries; ++k) {
                const bool m = pend[k] && lab[k] == key;
                s += m ? w[k] : 0.f;
                pend[k] = pend[k] && !m;
            }
            const float tot = wave_sum(s);
            if (r < (u32)kMaskSlots) {
#pragma unroll
                for (int j = 0; j < kMaskSlots; ++j)
                    if (r == (u32)j)
                        key_s[j] = key, sum_s[j] = tot;
            } else {
                if (lane == 0)
                    s_key[wave][r - kMaskSlots] = key, s_sum[wave][r - kMaskSlots] = tot;
                dsp += tot;
            }
            ++r;
        }
        if (lane == 0 && pos < n_isect) {
            slot_lab[pos] = make_int4(key_s[0], key_s[1], key_s[2], key_s[3]);
            slot_sum[pos] = make_float4(sum_s[0], sum_s[1], sum_s[2], sum_s[3]);
        }
        if (r <= (u32)kMaskSlots)
            continue;
        // spill: sum_k s_k E[k, :] over the pairs beyond the slots, D atomics into F[gid, :]
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        const u32 nsp = r - kMaskSlots;
        if (lane == 0) {
            if (d)
                atomicAdd(d + gid, dsp * scale_d);
            if (n_spilled)
                atomicAdd(n_spilled, 1u);
        }
        float *Fg = F + (int64_t)gid * D;
        for (int c0 = 0; c0 < D; c0 += 256) {
            const int c = c0 + lane * 4;
            if (c >= D)
                continue;
            f4 acc = f4{0.f, 0.f, 0.f, 0.f};
            for (u32 j = 0; j < nsp; ++j) {
                const int key = s_key[wave][j];
                if (key < 0)
                    continue;
                const float sj = s_sum[wave][j];
                const f4 t = load_tok<MT>(table + (int64_t)key * ts_row + c);
                acc.x = __builtin_fmaf(sj, t.x, acc.x);
                acc.y = __builtin_fmaf(sj, t.y, acc.y);
                acc.z = __builtin_fmaf(sj, t.z, acc.z);
                acc.w = __builtin_fmaf(sj, t.w, acc.w);
            }
            atomicAdd(Fg + c + 0, acc.x * scale_f);
            atomicAdd(Fg + c + 1, acc.y * scale_f);
            atomicAdd(Fg + c + 2, acc.z * scale_f);
            atomicAdd(Fg + c + 3, acc.w * scale_f);
        }
        // (the next record's list writes come after these reads in the wave's program order)
        __builtin_amdgcn_wave_barrier();
    }
}

#ifndef GWBP_MASK_FLIGHT
#define GWBP_MASK_FLIGHT 4
#endif
constexpr int kMaskFlight = GWBP_MASK_FLIGHT; // distinct labels whose table rows a wave reads together (NC <= 2; 2 above)

template <int NC, bool FULL, int MT>
__global__ __launch_bounds__(64 * kMaskWaves) void k_mask_apply(MaskApplyArgs A)
{
    typedef typename MapElem<MT>::raw TR;
    constexpr int FLIGHT = NC <= 2 ? kMaskFlight : 2;
    const TR *const table = static_cast<const TR *>(A.table);
    const u32 kind = A.ctr->blend_kind;
    if (kind == kBlendFused || kind == kBlendToken) {
        if (blockIdx.x == 0 && threadIdx.x == 0)
            atomicOr(&A.ctr->overflow, kOverflowMismatch);
        return;
    }
    if (A.ctr->overflow & 1u)
        return; // no emit positions (see k_mask_reduce)
    const int lane = (int)(threadIdx.x & 63u), wave = (int)uniform(threadIdx.x >> 6);
    u32 m_gid = 0, m_cnt = 0, m_es = 0;
    {
        const int64_t i0 = ((int64_t)blockIdx.x * kMaskWaves + wave) * kMaskPerWave;
        if (lane < kMaskPerWave && i0 + lane < A.N) {
            m_gid = A.order[i0 + lane];
            m_cnt = A.touched[m_gid];
            if (m_cnt)
                m_es = A.estart[m_gid];
        }
    }
    const int quad = lane & 3, sl = lane >> 2; // lane = (emit position within a batch of 16, slot)
    // which of the wave's Gaussians have weight at all, lane-parallel over their first 16 emit positions (as k_token_apply)
    u64 mine = __ballot(m_cnt != 0u);
    if (mine != 0ull) {
        const u32 last = m_cnt ? min(m_cnt, 16u) - 1u : 0u;
        const float4 *s4 = reinterpret_cast<const float4 *>(A.sums) + m_es;
        float4 v[16];
#pragma unroll
        for (int i = 0; i < 16; ++i)
            v[i] = s4[min((u32)i, last)];
        u32 bits = 0u;
#pragma unroll
        for (int i = 0; i < 16; ++i)
            bits |= (__float_as_uint(v[i].x) | __float_as_uint(v[i].y) | __float_as_uint(v[i].z) | __float_as_uint(v[i].w)) &
                    0x7FFFFFFFu;
        mine = __ballot(m_cnt != 0u && (m_cnt > 16u || bits != 0u));
    }
    constexpr int kCW = kTokCh * NC;
    const float *dsrc = A.d ? A.d : A.sums;
    for (int pass = 0; pass < A.n_pass; ++pass) {
        const int cbase = pass * kCW;
        u64 rest = mine;
        if (rest == 0ull)
            break;
        bool valid[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c)
            valid[c] = FULL || cbase + c * kTokCh + lane * 4 < A.D;
        const TR *tbase = table + (size_t)cbase + (size_t)lane * 4;
        // one batch of 16 emit positions x 4 slots (one (label, sum) per lane) into acc: equal labels merged first
        auto batch = [&](float om, int lab, f4 (&acc)[NC], float &dsum) {
            dsum += om;
            u64 todo = __ballot(om != 0.f && lab >= 0);
            while (todo != 0ull) {
                f4 t[FLIGHT][NC];
                float w[FLIGHT];
#pragma unroll
                for (int u = 0; u < FLIGHT; ++u) {
                    w[u] = 0.f;
                    if (todo != 0ull) { // wave-uniform
                        const int key = __builtin_amdgcn_readlane(lab, __ffsll((long long)todo) - 1);
                        const u64 m = todo & __ballot(lab == key);
                        todo &= ~m;
                        w[u] = wave_sum(((m >> lane) & 1ull) ? om : 0.f);
                        const TR *row = tbase + (int64_t)key * A.ts_row;
#pragma unroll
                        for (int c = 0; c < NC; ++c) {
                            t[u][c] = f4{0.f, 0.f, 0.f, 0.f};
                            if (valid[c])
                                t[u][c] = load_tok<MT>(row + c * kTokCh);
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < FLIGHT; ++u)
                    if (w[u] != 0.f) { // (wave-uniform; an unused slot must not turn 0 x NaN into NaN)
#pragma unroll
                        for (int c = 0; c < NC; ++c) {
                            acc[c].x = __builtin_fmaf(w[u], t[u][c].x, acc[c].x);
                            acc[c].y = __builtin_fmaf(w[u], t[u][c].y, acc[c].y);
                            acc[c].z = __builtin_fmaf(w[u], t[u][c].z, acc[c].z);
                            acc[c].w = __builtin_fmaf(w[u], t[u][c].w, acc[c].w);
                        }
                    }
            }
        };
        auto pop = [&]() -> int {
            if (rest == 0ull)
                return -1;
            const int k = __ffsll((long long)rest) - 1;
            rest &= rest - 1;
            return k;
        };
        // (first slots, row, d) of a Gaussian, requested without conditions
        auto request = [&](int k, float &om, int &lb, f4 (&fold)[NC], float &dv) {
            const u32 cnt = (u32)__builtin_amdgcn_readlane((int)m_cnt, k), es = (u32)__builtin_amdgcn_readlane((int)m_es, k);
            const u32 gid = (u32)__builtin_amdgcn_readlane((int)m_gid, k);
            const size_t at = (size_t)(es + min((u32)sl, cnt - 1u)) * kMaskSlots + quad;
            om = A.sums[at];
            lb = A.labels[at];
            const float *row = A.F + (size_t)gid * (size_t)A.D + (size_t)cbase + (size_t)lane * 4;
#pragma unroll
            for (int c = 0; c < NC; ++c)
                if (valid[c])
                    fold[c] = __builtin_nontemporal_load(reinterpret_cast<const f4 *>(row + c * kTokCh));
            dv = dsrc[A.d ? gid : 0u];
        };
        auto step = [&](int kc, float om_c, int lb_c, f4 (&fold_c)[NC], float d_c, float &om_n, int &lb_n, f4 (&fold_n)[NC],
                        float &d_n) -> int {
            const int kn = pop();
            request(kn >= 0 ? kn : kc, om_n, lb_n, fold_n, d_n);
            const u32 gid = (u32)__builtin_amdgcn_readlane((int)m_gid, kc), cnt = (u32)__builtin_amdgcn_readlane((int)m_cnt, kc);
            const u32 es = (u32)__builtin_amdgcn_readlane((int)m_es, kc);
            f4 acc[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c)
                acc[c] = f4{0.f, 0.f, 0.f, 0.f};
            float dsum = 0.f;
            bool any = false;
            {
                const float om = (u32)sl < cnt ? om_c : 0.f;
                if (__ballot(om != 0.f) != 0ull) {
                    any = true;
                    batch(om, lb_c, acc, dsum);
                }
            }
            for (u32 s0 = 16u; s0 < cnt; s0 += 16u) { // rectangles of more than 16 tiles
                const u32 slot = s0 + (u32)sl;
                const size_t at = (size_t)(es + slot) * kMaskSlots + quad;
                const float om = slot < cnt ? A.sums[at] : 0.f;
                if (__ballot(om != 0.f) == 0ull)
                    continue;
                any = true;
                batch(om, slot < cnt ? A.labels[at] : -1, acc, dsum);
            }
            if (any) {
                float *frow = A.F + (size_t)gid * (size_t)A.D + (size_t)cbase + (size_t)lane * 4;
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    f4 r = fold_c[c];
                    r.x = __builtin_fmaf(A.scale_f, acc[c].x, r.x);
                    r.y = __builtin_fmaf(A.scale_f, acc[c].y, r.y);
                    r.z = __builtin_fmaf(A.scale_f, acc[c].z, r.z);
                    r.w = __builtin_fmaf(A.scale_f, acc[c].w, r.w);
                    if (valid[c])
                        __builtin_nontemporal_store(r, reinterpret_cast<f4 *>(frow + c * kTokCh));
                }
                if (pass == 0 && A.d) { // the wave owns d[gid] as well: plain read-modify-write
                    const float tot = wave_sum(dsum);
                    if (lane == 0)
                        A.d[gid] = __builtin_fmaf(A.scale_d, tot, d_c);
                }
            }
            return kn;
        };
        int kc = pop();
        float om_a, om_b, d_a, d_b;
        int lb_a, lb_b;
        f4 fold_a[NC], fold_b[NC];
        request(kc, om_a, lb_a, fold_a, d_a);
        for (;;) {
            kc = step(kc, om_a, lb_a, fold_a, d_a, om_b, lb_b, fold_b, d_b);
            if (kc < 0)
                break;
            kc = step(kc, om_b, lb_b, fold_b, d_b, om_a, lb_a, fold_a, d_a);
            if (kc < 0)
                break;
        }
    }
}

template <typename T, int MT>
static void launch_reduce_t(const Ws &W, const ViewDev &V, const void *labels, int64_t ls_y, int64_t ls_x, const int32_t *ymap,
                            const int32_t *xmap, int M, const void *table, int64_t ts_row, int D, float scale_f, float scale_d,
                            float *F, float *d, const MaskSlots &S, u32 *n_spilled, hipStream_t s)
{
    const int n_tiles = V.tile_w * V.tile_h;
    hipLaunchKernelGGL((k_mask_reduce<T, MT>), dim3(n_tiles), dim3(kMaskThreads), 0, s, V, W.tile_order, W.tile_offsets,
                       W.hdr_count, W.headers, W.wpool, W.dkeys[1], W.rect, static_cast<const T *>(labels), ls_y, ls_x, ymap, xmap,
                       M, table, ts_row, D, scale_f, scale_d, F, d, S.labels, S.sums, n_spilled, W.counters);
}

template <int MT>
static void launch_reduce_mt(int label_type, const Ws &W, const ViewDev &V, const void *labels, int64_t ls_y, int64_t ls_x,
                             const int32_t *ymap, const int32_t *xmap, int M, const void *table, int64_t ts_row, int D,
                             float scale_f, float scale_d, float *F, float *d, const MaskSlots &S, u32 *n_spilled, hipStream_t s)
{
    if (label_type == GWBP_LABEL_U8)
        launch_reduce_t<uint8_t, MT>(W, V, labels, ls_y, ls_x, ymap, xmap, M, table, ts_row, D, scale_f, scale_d, F, d, S,
                                     n_spilled, s);
    else if (label_type == GWBP_LABEL_I16)
        launch_reduce_t<int16_t, MT>(W, V, labels, ls_y, ls_x, ymap, xmap, M, table, ts_row, D, scale_f, scale_d, F, d, S,
                                     n_spilled, s);
    else
        launch_reduce_t<int32_t, MT>(W, V, labels, ls_y, ls_x, ymap, xmap, M, table, ts_row, D, scale_f, scale_d, F, d, S,
                                     n_spilled, s);
}

template <int MT>
static void launch_apply_mt(const MaskApplyArgs &A, int nc, bool full, dim3 grid, hipStream_t s)
{
    const dim3 block(64 * kMaskWaves);
#define GWBP_MASK_LAUNCH(NCV)                                                                                                  \
    do {                                                                                                                       \
        if (full)                                                                                                              \
            hipLaunchKernelGGL((k_mask_apply<NCV, true, MT>), grid, block, 0, s, A);                                           \
        else                                                                                                                   \
            hipLaunchKernelGGL((k_mask_apply<NCV, false, MT>), grid, block, 0, s, A);                                          \
    } while (0)
    if (nc == 4)
        GWBP_MASK_LAUNCH(4);
    else if (nc == 3)
        GWBP_MASK_LAUNCH(3);
    else if (nc == 2)
        GWBP_MASK_LAUNCH(2);
    else
        GWBP_MASK_LAUNCH(1);
#undef GWBP_MASK_LAUNCH
}

int launch_mask_features(const Layout &L, const Ws &W, const ViewDev &V, const void *labels, int label_type, int64_t ls_y,
                         int64_t ls_x, const int32_t *ymap, const int32_t *xmap, const void *table, int table_type,
                         int64_t ts_row, int M, int D, float scale_f, float scale_d, float *F, float *d, const MaskSlots &S,
                         u32 *n_spilled, hipStream_t s)
{
    if (L.n == 0)
        return GWBP_OK;
    hipLaunchKernelGGL(k_zero_mask_sums, dim3(1024), dim3(256), 0, s, S.sums, W.counters);
    with_map_type(table_type, [&](auto MT) {
        launch_reduce_mt<MT>(label_type, W, V, labels, ls_y, ls_x, ymap, xmap, M, table, ts_row, D, scale_f, scale_d, F, d, S, n_spilled, s);
    });
    int rc = check_hip(hipGetLastError(), "mask_reduce launch");
    if (rc)
        return rc;
    MaskApplyArgs A;
    A.N = L.n, A.order = W.dvals[0], A.touched = W.touched, A.estart = W.dkeys[1];
    A.labels = reinterpret_cast<const int *>(S.labels), A.sums = reinterpret_cast<const float *>(S.sums);
    A.table = table, A.ts_row = ts_row, A.D = D, A.scale_f = scale_f, A.scale_d = scale_d, A.F = F, A.d = d, A.ctr = W.counters;
    // 256-channel chunks: as few passes as four chunks side by side allow (k_token_apply's split)
    const int n_chunk = (D + kTokCh - 1) / kTokCh;
    A.n_pass = (n_chunk + 3) / 4;
    const int nc = (n_chunk + A.n_pass - 1) / A.n_pass;
    const bool full = D % kTokCh == 0 && n_chunk == A.n_pass * nc;
    const int64_t blocks = (L.n + kMaskGroup - 1) / kMaskGroup;
    if (blocks > 0x7FFFFFFFll)
        return set_error(GWBP_EINVAL, "gwbp_scatter_mask_features: grid too large");
    const dim3 grid((unsigned)blocks);
    with_map_type(table_type, [&](auto MT) { launch_apply_mt<MT>(A, nc, full, grid, s); });
    return check_hip(hipGetLastError(), "mask_apply launch");
}

} // namespace gwbp
