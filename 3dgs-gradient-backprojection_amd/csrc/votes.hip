// votes.hip -- 3-D masks from 2-D label maps by per-view VOTING (the binary and projection votes of a masklet lift):
//     C[g, k] += 1 per view in which g casts a vote for label k,     n[g] += 1 per view in which g votes at all
//
// k_vote_labels (binary vote): one workgroup per tile (heaviest tile lists first), four waves, one (Gaussian, tile) record per wave
//   at a time, over the weight store of gwbp_blend_weights* -- the walk of k_scatter_labels (label.hip), whose tile label staging is
//   repeated here.  Every entry with w > 0 sets bit 0 ("seen") and, when its label k is in [0, K), bit k + 1 of the Gaussian's
//   row of a per-view bitset seen[N][words], words = ceil((K + 1) / 32).  Reduce by key: round 0 takes word 0 (it always carries
//   bit 0), every later round the word of the first pending entry of the first lane that has one; the matching bits are ORed
//   across the wave (DPP) and ONE no-return atomicOr per non-zero word per record sets them.  A record needs at most `words`
//   rounds; no float atomic runs here.
// k_vote_commit: one thread per (Gaussian, word), launched behind k_vote_labels on the same stream: every set label bit adds 1 to
//   its column of C, bit 0 adds 1 to n, and the word is written back to 0 -- the bitset is clean for the next view with no memset.
//   The adds are float atomics: several workspaces may commit different views into one C and n at once.  Counts stay exact up to
//   2^24 views.
// Why a bitset per view and not a per-(Gaussian, label) stamp of the last view that voted: two workspaces working on views v and
// v + 1 at once would count one Gaussian twice; each workspace's bitset only ever holds the view it is working on.
//
// k_vote_projected (projection vote): one thread per Gaussian over the projected table of gwbp_project (no sort, no blend).  A
//   Gaussian with radius > 0 whose rounded centre (rintf: round half to even) lies inside the image votes once, for the label of
//   that pixel: C[g, L(y, x)] += 1 when the label is in [0, K), n[g] += 1 in any case -- unless a pixel weight map is given and
//   its value there is not > 0 (then the Gaussian casts no vote in this view).
#include "gwbp_dev.h"

namespace gwbp {

constexpr int kVoteThreads = 256; // one workgroup per tile, four waves
constexpr int kVoteSlots = 4;     // a record holds at most 256 entries: four per lane
constexpr int kCommitThreads = 256;

// OR over the 64 lanes, returned wave-uniform: the DPP steps of wave_sum (gwbp_dev.h) with | for +.
template <int CTRL>
__device__ __forceinline__ u32 dpp_u(u32 x)
{
    return (u32)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xF, 0xF, true);
}
__device__ __forceinline__ u32 wave_or(u32 v)
{
    v |= dpp_u<0xB1>(v);  // quad_perm [1,0,3,2]
    v |= dpp_u<0x4E>(v);  // quad_perm [2,3,0,1]
    v |= dpp_u<0x141>(v); // row_half_mirror
    v |= dpp_u<0x140>(v); // row_mirror
    const u32 r0 = (u32)__builtin_amdgcn_readlane((int)v, 0), r1 = (u32)__builtin_amdgcn_readlane((int)v, 16);
    const u32 r2 = (u32)__builtin_amdgcn_readlane((int)v, 32), r3 = (u32)__builtin_amdgcn_readlane((int)v, 48);
    return (r0 | r1) | (r2 | r3);
}

template <typename T>
__global__ __launch_bounds__(kVoteThreads) void k_vote_labels(
    ViewDev V, const u32 *__restrict__ tile_order, const u32 *__restrict__ tile_offsets, const u32 *__restrict__ hdr_count,
    const Header *__restrict__ headers, const WPair *__restrict__ wpool, const T *__restrict__ labels, int64_t ls_y, int64_t ls_x,
    const int32_t *__restrict__ ymap, const int32_t *__restrict__ xmap, int K, int words, u32 *__restrict__ seen,
    Counters *__restrict__ ctr)
{
    const u32 kind = ctr->blend_kind;
    if (kind == kBlendFused || kind == kBlendToken) { // the workspace holds no weight store: refuse, flag (as k_scatter_labels does)
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
        const int p = threadIdx.x; // kVoteThreads == kTilePix
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

    for (u32 h = wave; h < nh; h += kVoteThreads / 64) {
        const Header *hp = hb + h;
        const u32 gid = uniform(hp->gid), w0 = uniform(hp->woff[0]), w2 = uniform(hp->woff[2]);
        const u32 counts = uniform(hp->counts);
        const u32 n01 = (counts & 0xFFu) + ((counts >> 8) & 0xFFu);
        const u32 n = n01 + ((counts >> 16) & 0xFFu) + (counts >> 24);
        u32 *row = seen + (size_t)gid * (size_t)words;

        int word[kVoteSlots]; // the bitset word of the entry's label bit (label k -> bit k + 1), -1 = no label bit
        u32 bit[kVoteSlots];
        bool voted = false;
#pragma unroll
        for (int k = 0; k < kVoteSlots; ++k) {
            word[k] = -1, bit[k] = 0u;
            const u32 i = (u32)(k * 64 + lane);
            if ((u32)(k * 64) < n && i < n) {
                const WPair e = wpool[i < n01 ? w0 + i : w2 + (i - n01)];
                if (e.w > 0.f) { // (a stored entry's pixel is < 256; only padding carries kPadPix, and it is not read)
                    voted = true;
                    const int lab = s_lab[e.pix];
                    if (lab >= 0)
                        word[k] = (lab + 1) >> 5, bit[k] = 1u << ((lab + 1) & 31);
                }
            }
        }
        if (__builtin_amdgcn_ballot_w64(voted) == 0ull)
            continue; // (entries of weight <= 0: a pixel weight map's zero or negative values cast no vote)

        for (int key = 0;;) { // round 0: word 0, which carries the "seen" bit
            u32 m = 0u;
#pragma unroll
            for (int k = 0; k < kVoteSlots; ++k) {
                const bool hit = word[k] == key;
                m |= hit ? bit[k] : 0u;
                word[k] = hit ? -1 : word[k];
            }
            m = wave_or(m);
            if (key == 0)
                m |= 1u;
            if (lane == 0)
                atomicOr(row + key, m);
            u64 any = 0ull;
#pragma unroll
            for (int k = 0; k < kVoteSlots; ++k)
                any |= __builtin_amdgcn_ballot_w64(word[k] >= 0);
            if (any == 0ull)
                break;
            int cand = -1; // this lane's first pending word
#pragma unroll
            for (int k = kVoteSlots - 1; k >= 0; --k)
                cand = word[k] >= 0 ? word[k] : cand;
            key = __builtin_amdgcn_readlane(cand, (int)__builtin_ctzll(any));
        }
    }
}

__global__ __launch_bounds__(kCommitThreads) void k_vote_commit(int64_t n_words, int words, int K, u32 *__restrict__ seen,
                                                                 float *__restrict__ C, int64_t ldc, float *__restrict__ n)
{
    const int64_t i = (int64_t)blockIdx.x * kCommitThreads + threadIdx.x;
    if (i >= n_words)
        return;
    u32 m = seen[i];
    if (m == 0u)
        return;
    seen[i] = 0u;
    const int64_t g = i / words;
    const int wi = (int)(i - g * words);
    if (wi == 0) {
        if (n)
            atomicAdd(n + g, 1.0f);
        m &= ~1u;
    }
    float *Cg = C + g * ldc;
    while (m) {
        const int b = __builtin_ctz(m);
        m &= m - 1u;
        const int k = wi * 32 + b - 1;
        if (k < K) // (k_vote_labels sets no bit beyond K; the test keeps a stray bit from writing past the row)
            atomicAdd(Cg + k, 1.0f);
    }
}

// c(x, y) of a per-pixel weight map (PixW, gwbp_dev.h); GWBP_PIXW_U8 reads any non-zero byte as 1
__device__ __forceinline__ float pixel_weight(const PixW &pw, int x, int y)
{
    const int64_t off = (int64_t)y * pw.ws_y + (int64_t)x * pw.ws_x;
    switch (pw.dtype) {
    case GWBP_PIXW_U8:
        return static_cast<const unsigned char *>(pw.data)[off] != 0 ? 1.0f : 0.0f;
    case GWBP_PIXW_F16:
        return MapElem<GWBP_MAP_F16>::cvt(static_cast<const unsigned short *>(pw.data)[off]);
    case GWBP_PIXW_BF16:
        return MapElem<GWBP_MAP_BF16>::cvt(static_cast<const unsigned short *>(pw.data)[off]);
    default:
        return static_cast<const float *>(pw.data)[off];
    }
}

template <typename T>
__global__ __launch_bounds__(kCommitThreads) void k_vote_projected(
    int64_t N, int W, int H, const G2D *__restrict__ g2d, const T *__restrict__ labels, int64_t ls_y, int64_t ls_x,
    const int32_t *__restrict__ ymap, const int32_t *__restrict__ xmap, PixW pw, int K, float *__restrict__ C, int64_t ldc,
    float *__restrict__ n)
{
    const int64_t g = (int64_t)blockIdx.x * kCommitThreads + threadIdx.x;
    if (g >= N)
        return;
    const float4 a = reinterpret_cast<const float4 *>(g2d + g)[1]; // (ca, cb, cc, radius)
    if (__float_as_int(a.w) <= 0)
        return;
    const float4 m = reinterpret_cast<const float4 *>(g2d + g)[0]; // (mx, my, opac, depth)
    const float fx = __builtin_rintf(m.x), fy = __builtin_rintf(m.y);
    if (!(fx >= 0.0f && fx < (float)W && fy >= 0.0f && fy < (float)H)) // (also false for a NaN centre)
        return;
    const int x = (int)fx, y = (int)fy;
    if (pw.data && !(pixel_weight(pw, x, y) > 0.0f))
        return;
    const int64_t row = ymap ? ymap[y] : y, col = xmap ? xmap[x] : x;
    const int lab = (int)labels[row * ls_y + col * ls_x];
    if (lab >= 0 && lab < K)
        atomicAdd(C + g * ldc + lab, 1.0f);
    if (n)
        atomicAdd(n + g, 1.0f);
}

static int vote_words(int K) { return (int)(((int64_t)K + 1 + 31) / 32); }

template <typename T>
static void launch_vote_labels_t(const Layout &L, const Ws &W, const ViewDev &V, const void *labels, int64_t ls_y, int64_t ls_x,
                                 const int32_t *ymap, const int32_t *xmap, int K, u32 *seen, hipStream_t s)
{
    const int n_tiles = V.tile_w * V.tile_h;
    hipLaunchKernelGGL(k_vote_labels<T>, dim3(n_tiles), dim3(kVoteThreads), 0, s, V, W.tile_order, W.tile_offsets, W.hdr_count,
                       W.headers, W.wpool, static_cast<const T *>(labels), ls_y, ls_x, ymap, xmap, K, vote_words(K), seen,
                       W.counters);
}

int launch_vote_labels(const Layout &L, const Ws &W, const ViewDev &V, const void *labels, int label_type, int64_t ls_y,
                       int64_t ls_x, const int32_t *ymap, const int32_t *xmap, int K, u32 *seen, float *C, int64_t ldc, float *n,
                       hipStream_t s)
{
    if (label_type == GWBP_LABEL_U8)
        launch_vote_labels_t<uint8_t>(L, W, V, labels, ls_y, ls_x, ymap, xmap, K, seen, s);
    else if (label_type == GWBP_LABEL_I16)
        launch_vote_labels_t<int16_t>(L, W, V, labels, ls_y, ls_x, ymap, xmap, K, seen, s);
    else
        launch_vote_labels_t<int32_t>(L, W, V, labels, ls_y, ls_x, ymap, xmap, K, seen, s);
    int rc = check_hip(hipGetLastError(), "vote_labels launch");
    if (rc || L.n == 0)
        return rc;
    const int words = vote_words(K);
    const int64_t n_words = L.n * (int64_t)words;
    const int64_t blocks = (n_words + kCommitThreads - 1) / kCommitThreads;
    hipLaunchKernelGGL(k_vote_commit, dim3((unsigned)blocks), dim3(kCommitThreads), 0, s, n_words, words, K, seen, C, ldc, n);
    return check_hip(hipGetLastError(), "vote_commit launch");
}

int launch_vote_projected(const Layout &L, const Ws &W, const ViewDev &V, const void *labels, int label_type, int64_t ls_y,
                          int64_t ls_x, const int32_t *ymap, const int32_t *xmap, const PixW *pw, int K, float *C, int64_t ldc,
                          float *n, hipStream_t s)
{
    if (L.n == 0)
        return GWBP_OK;
    PixW P = pw ? *pw : PixW{nullptr, 0, 0, GWBP_PIXW_F32};
    const dim3 grid((unsigned)((L.n + kCommitThreads - 1) / kCommitThreads)), block(kCommitThreads);
    if (label_type == GWBP_LABEL_U8)
        hipLaunchKernelGGL(k_vote_projected<uint8_t>, grid, block, 0, s, L.n, V.W, V.H, W.g2d,
                           static_cast<const uint8_t *>(labels), ls_y, ls_x, ymap, xmap, P, K, C, ldc, n);
    else if (label_type == GWBP_LABEL_I16)
        hipLaunchKernelGGL(k_vote_projected<int16_t>, grid, block, 0, s, L.n, V.W, V.H, W.g2d,
                           static_cast<const int16_t *>(labels), ls_y, ls_x, ymap, xmap, P, K, C, ldc, n);
    else
        hipLaunchKernelGGL(k_vote_projected<int32_t>, grid, block, 0, s, L.n, V.W, V.H, W.g2d,
                           static_cast<const int32_t *>(labels), ls_y, ls_x, ymap, xmap, P, K, C, ldc, n);
    return check_hip(hipGetLastError(), "vote_projected launch");
}

} // namespace gwbp
