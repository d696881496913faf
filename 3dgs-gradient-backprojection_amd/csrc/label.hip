// label.hip -- back-projection of an integer LABEL map (a segmenter's class / instance ids, a binary mask):
//     F[g, k] += scale_f * sum_p w_g(p) * [L(p) == k],     d[g] += scale_d * sum_p w_g(p)
// i.e. gwbp_scatter on one_hot(L, K) without the [H, W, K] map and without the K - n zero columns of every record's row.  A label
// outside [0, K) adds to no column of F (an all-zero one-hot row) but its weight still counts in d.
//
// k_scatter_labels: one workgroup per tile (heaviest tile lists first), four waves, one (Gaussian, tile) record per wave at a time.
//   - the tile's 256 labels are staged once in LDS as int32 (-1 = ignored); low-resolution maps go through the int32 nearest-index
//     maps of gwbp_scatter_upsampled while they are staged
//   - a record's entries (at most 256: four per lane) are read as two dense runs, quarters 0|1 at woff[0] and 2|3 at woff[2], so
//     the padding the 256-channel kernel wants between the halves is never touched; each lane looks its pixels' labels up in LDS
//   - reduce by key: a leader label (the first pending entry of the first lane that has one, v_readlane) is matched by every lane,
//     the matching weights are summed across the wave (DPP), and the sum becomes ONE lane of a batch of adds.  After kLabelRounds
//     leaders the entries still pending add their own weights, one wave instruction per slot of four: a per-pixel-random map costs
//     an atomic per entry, not a serial loop
//   - the batch: lane i of a wave register pair holds the i-th (address, value) the wave has produced -- label sums and the
//     record's d share of several records -- and ONE no-return global_atomic_add_f32 issues them all when it is nearly full
// Cost model: the weight store is read once (8 B per pair) and the adds are few; the float atomic unit sees
// one 4-B add per (record, distinct label), not K of them.
#include "gwbp_dev.h"

namespace gwbp {

constexpr int kLabelThreads = 256; // one workgroup per tile, four waves
constexpr int kLabelRounds = 4;    // leader rounds per record; what is left after them adds entry by entry
constexpr int kLabelSlots = 4;     // a record holds at most 256 entries: four per lane

template <typename T>
__global__ __launch_bounds__(kLabelThreads) void k_scatter_labels(
    ViewDev V, const u32 *__restrict__ tile_order, const u32 *__restrict__ tile_offsets, const u32 *__restrict__ hdr_count,
    const Header *__restrict__ headers, const WPair *__restrict__ wpool, const T *__restrict__ labels, int64_t ls_y, int64_t ls_x,
    const int32_t *__restrict__ ymap, const int32_t *__restrict__ xmap, int K, float scale_f, float scale_d, float *__restrict__ F,
    int64_t ldf, float *__restrict__ d, Counters *__restrict__ ctr)
{
    const u32 kind = ctr->blend_kind;
    if (kind == kBlendFused || kind == kBlendToken) { // the workspace holds no weight store: refuse, flag (as k_token_apply does)
        if (blockIdx.x == 0 && threadIdx.x == 0)
            atomicOr(&ctr->overflow, kOverflowMismatch);
        return;
    }
    const int tile = (int)tile_order[blockIdx.x];
    const u32 nh = hdr_count[tile];
    if (nh == 0)
        return;
    const int tx = tile % V.tile_w, ty = tile / V.tile_w;

    __shared__ int s_lab[kTilePix];
    {
        const int p = threadIdx.x; // kLabelThreads == kTilePix
        const int ix = tx * kTile + (p & 15), iy = ty * kTile + (p >> 4);
        int lab = -1;
        if (ix < V.W && iy < V.H) {
            const int64_t row = ymap ? ymap[iy] : iy, col = xmap ? xmap[ix] : ix;
            const int v = (int)labels[row * ls_y + col * ls_x];
            lab = (v >= 0 && v < K) ? v : -1;
        }
        s_lab[p] = lab;
    }
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const u32 wave = uniform(threadIdx.x >> 6);
    const Header *hb = headers + tile_offsets[tile];
    // the batch of adds: lane i holds the i-th (address, value) of this wave; n_out is wave-uniform
    float *out_p = F;
    float out_v = 0.f;
    u32 n_out = 0;
    auto stage = [&](float *addr, float v) {
        if ((u32)lane == n_out)
            out_p = addr, out_v = v;
        ++n_out;
    };
    auto flush = [&]() {
        if ((u32)lane < n_out)
            atomicAdd(out_p, out_v);
        n_out = 0;
    };

    for (u32 h = wave; h < nh; h += kLabelThreads / 64) {
        if (n_out > 64u - (kLabelRounds + 1)) // a record stages at most kLabelRounds label sums and its d share
            flush();
        const Header *hp = hb + h;
        const u32 gid = uniform(hp->gid), w0 = uniform(hp->woff[0]), w2 = uniform(hp->woff[2]);
        const u32 counts = uniform(hp->counts);
        const u32 n01 = (counts & 0xFFu) + ((counts >> 8) & 0xFFu);
        const u32 n = n01 + ((counts >> 16) & 0xFFu) + (counts >> 24);
        float *Fg = F + (int64_t)gid * ldf;

        int lab[kLabelSlots];
        float w[kLabelSlots];
        bool pend[kLabelSlots];
        float wl = 0.f;
#pragma unroll
        for (int k = 0; k < kLabelSlots; ++k) {
            lab[k] = -1, w[k] = 0.f;
            const u32 i = (u32)(k * 64 + lane);
            if ((u32)(k * 64) < n && i < n) {
                const WPair e = wpool[i < n01 ? w0 + i : w2 + (i - n01)];
                w[k] = e.w;
                lab[k] = s_lab[e.pix]; // (a stored entry's pixel is < 256; only padding carries kPadPix, and it is not read)
            }
            wl += w[k];
            pend[k] = lab[k] >= 0;
        }
        if (d)
            stage(d + gid, wave_sum(wl) * scale_d);

        for (int r = 0; r < kLabelRounds; ++r) {
            u64 any = 0ull;
#pragma unroll
            for (int k = 0; k < kLabelSlots; ++k)
                any |= __builtin_amdgcn_ballot_w64(pend[k]);
            if (any == 0ull)
                break;
            int cand = -1; // this lane's first pending label
#pragma unroll
            for (int k = kLabelSlots - 1; k >= 0; --k)
                cand = pend[k] ? lab[k] : cand;
            const int key = __builtin_amdgcn_readlane(cand, (int)__builtin_ctzll(any));
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < kLabelSlots; ++k) {
                const bool m = pend[k] && lab[k] == key;
                s += m ? w[k] : 0.f;
                pend[k] = pend[k] && !m;
            }
            stage(Fg + key, wave_sum(s) * scale_f);
        }
        // more distinct labels than leader rounds: every entry still pending adds its own weight (one instruction per slot)
#pragma unroll
        for (int k = 0; k < kLabelSlots; ++k)
            if (__builtin_amdgcn_ballot_w64(pend[k]) != 0ull && pend[k])
                atomicAdd(Fg + lab[k], w[k] * scale_f);
    }
    flush();
}

template <typename T>
static void launch_labels_t(const Layout &L, const Ws &W, const ViewDev &V, const void *labels, int64_t ls_y, int64_t ls_x,
                            const int32_t *ymap, const int32_t *xmap, int K, float scale_f, float scale_d, float *F, int64_t ldf,
                            float *d, hipStream_t s)
{
    (void)L;
    const int n_tiles = V.tile_w * V.tile_h;
    hipLaunchKernelGGL(k_scatter_labels<T>, dim3(n_tiles), dim3(kLabelThreads), 0, s, V, W.tile_order, W.tile_offsets, W.hdr_count,
                       W.headers, W.wpool, static_cast<const T *>(labels), ls_y, ls_x, ymap, xmap, K, scale_f, scale_d, F, ldf, d,
                       W.counters);
}

int launch_scatter_labels(const Layout &L, const Ws &W, const ViewDev &V, const void *labels, int label_type, int64_t ls_y,
                          int64_t ls_x, const int32_t *ymap, const int32_t *xmap, int K, float scale_f, float scale_d, float *F,
                          int64_t ldf, float *d, hipStream_t s)
{
    if (label_type == GWBP_LABEL_U8)
        launch_labels_t<uint8_t>(L, W, V, labels, ls_y, ls_x, ymap, xmap, K, scale_f, scale_d, F, ldf, d, s);
    else if (label_type == GWBP_LABEL_I16)
        launch_labels_t<int16_t>(L, W, V, labels, ls_y, ls_x, ymap, xmap, K, scale_f, scale_d, F, ldf, d, s);
    else
        launch_labels_t<int32_t>(L, W, V, labels, ls_y, ls_x, ymap, xmap, K, scale_f, scale_d, F, ldf, d, s);
    return check_hip(hipGetLastError(), "scatter_labels launch");
}

} // namespace gwbp
