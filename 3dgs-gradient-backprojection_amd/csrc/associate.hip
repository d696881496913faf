// associate.hip -- the integer walks of the weight store behind associate_masks (associate.py): which 3-D group does a mask
// of a new view continue?
//     overlap:  O[row(L(p)), group[g] + 1] += q(w)       one int64 table per view, "mask m x existing group j"
//     votes:    V[g, remap[L(p)]]          += q(w)       int64 [N, ldv], a Gaussian's evidence per group
//     sparse:   slot(g, remap[L(p)])       += q(w)       the votes into S (key, sum) slots per Gaussian instead of a dense row
// with q(w) = (uint32) rintf(fminf(fmaxf(w, 0), 4) * 2^20): every sum is an INTEGER sum, so the tables have the same bits whatever
// the order of the atomics, the split between the leader path and the left-over path, or what the LDS table combined first.  That
// is what a sequential association needs: each view's table decides the next view's input.
//
// assoc_walk<T, kMode>, the body of k_label_assoc<T, kVotes> and k_label_votes_sparse<T>: the walk of k_scatter_labels (label.hip)
// -- one workgroup per tile in tile_order, the tile's 256 labels staged once in LDS (through the nearest-index maps for a
// low-resolution map), a record's entries read as the two dense runs,
// reduce by key with kAssocRounds leaders and the left-over entries one by one.
//   - overlap: the staged value is the ROW (L(p), or num_labels for an ignored pixel: column sums stay complete); the column is
//     the record's.  Every workgroup would hit the same few hundred addresses of O, so the sums go into an LDS table keyed by
//     the element's offset row * ldo + col first -- open addressing, kAssocProbes probes, 64-bit LDS atomics -- and each occupied
//     slot is flushed with ONE 8-byte global atomic per workgroup.  An entry that finds no slot adds to O directly: the same
//     integer either way.  The leader sums of several records go into the table together, one lane each (the batch below)
//   - votes: the staged value is the COLUMN remap[L(p)] (-1: adds nothing).  Adds go to many rows: one 8-byte atomic per (record,
//     distinct column), batched as k_scatter_labels batches its float adds -- lane i holds the i-th (address, value) of the wave.
//   - sparse: the votes' walk; the destination is found, not computed.  A lane carries (row, key, value), probes the row's slots
//     0 .. S-1 in index order -- a relaxed agent-scope load of the key, a 4-byte compare-and-swap (empty -> key) only where the load
//     saw empty -- and adds with one 8-byte atomic to the slot whose key is its own, or to spill[row] after S misses.  A key never
//     changes once set, so a load can be stale only as "empty" (which costs the compare-and-swap, whose answer is the truth), and
//     a lane claims slot s only after it has SEEN another key in every slot before s: no key can sit in two slots of a row.
//     total[row] (optional) takes the record's whole sum, whatever the labels, as one more staged entry (key kAssocTotal).
// A record's per-key sum fits uint32 (256 entries x 2^22).  No float atomics; every loop is wave-uniform and bounded (the probe
// loop by S <= 32, left by a ballot as `combine`'s): no retry, no spin, no loop inside a divergent branch.
#include "gwbp_dev.h"

namespace gwbp {

constexpr int kAssocThreads = 256; // one workgroup per tile, four waves
constexpr int kAssocRounds = 4;    // leader rounds per record
constexpr int kAssocSlots = 4;     // a record holds at most 256 entries: four per lane
// the overlap table of one workgroup: a tile holds 256 pixels, so at most 256 rows; a few labels x a few groups is the common
// case and the table stays sparse.  Twice the worst row count keeps the probe sequences short; what does not fit goes to O.
constexpr int kAssocTable = 512;
constexpr int kAssocProbes = 8;
constexpr u64 kAssocEmpty = ~0ull; // (a key is an element's offset in O, below 2^63)
enum AssocMode { kAssocOverlap = 0, kAssocVotes = 1, kAssocSparse = 2 };
constexpr int kAssocTotal = -2;    // sparse: the staged key of a record's sum for total[] (a vote's key is >= 0)

// the per-Gaussian slot lists of gwbp_label_votes_sparse (include/gwbp.h): keys int32 [N, ldk] (-1 = empty), vals int64 [N, ldv],
// spill int64 [N], total int64 [N] or NULL
struct SparseDev {
    int32_t *keys;
    u64 *vals, *spill, *total;
    int64_t ldk, ldv;
    int slots;
};

__device__ __forceinline__ u32 assoc_quantize(float w)
{
    // fmaxf(NaN, 0) = 0; w * 2^20 is exact; rintf rounds to nearest, half to even
    return (u32)__builtin_rintf(__builtin_fminf(__builtin_fmaxf(w, 0.f), 4.f) * 1048576.f);
}

template <int CTRL>
__device__ __forceinline__ u32 dpp_u(u32 x)
{
    return (u32)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xF, 0xF, true);
}
// wave_sum (gwbp_dev.h) for integers: wave-uniform, every lane active
__device__ __forceinline__ u32 wave_sum_u32(u32 v)
{
    v += dpp_u<0xB1>(v);
    v += dpp_u<0x4E>(v);
    v += dpp_u<0x141>(v);
    v += dpp_u<0x140>(v);
    return (u32)__builtin_amdgcn_readlane((int)v, 0) + (u32)__builtin_amdgcn_readlane((int)v, 16) +
           (u32)__builtin_amdgcn_readlane((int)v, 32) + (u32)__builtin_amdgcn_readlane((int)v, 48);
}

// The walk, shared by the kernels below (a device function, so that k_label_assoc keeps its arguments and its code as they were).
// aux: group int32 [N] (overlap) or remap int32 [K] (votes, sparse); out: O int64 [K + 1, ld] or V int64 [N, ld]; sparse: SP
template <typename T, int kMode>
__device__ __forceinline__ void assoc_walk(
    const ViewDev &V, const u32 *__restrict__ tile_order, const u32 *__restrict__ tile_offsets, const u32 *__restrict__ hdr_count,
    const Header *__restrict__ headers, const WPair *__restrict__ wpool, const T *__restrict__ labels, int64_t ls_y, int64_t ls_x,
    const int32_t *__restrict__ ymap, const int32_t *__restrict__ xmap, int K, const int32_t *__restrict__ aux, int n_cols,
    u64 *__restrict__ out, int64_t ld, Counters *__restrict__ ctr, const SparseDev &SP)
{
    constexpr bool kSparse = kMode == kAssocSparse;
    constexpr bool kVotes = kMode != kAssocOverlap; // the votes' walk: the staged value is a column / key, adds go to row gid
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
    __shared__ u64 s_key[kVotes ? 1 : kAssocTable];
    __shared__ u64 s_val[kVotes ? 1 : kAssocTable];
    {
        const int p = threadIdx.x; // kAssocThreads == kTilePix
        const int ix = tx * kTile + (p & 15), iy = ty * kTile + (p >> 4);
        int lab = -1; // a pixel outside the image has no entry in the store
        if (ix < V.W && iy < V.H) {
            const int64_t row = ymap ? ymap[iy] : iy, col = xmap ? xmap[ix] : ix;
            const int v = (int)labels[row * ls_y + col * ls_x];
            const bool in = v >= 0 && v < K;
            if (kVotes) {
                const int c = in ? aux[v] : -1;
                lab = (c >= 0 && (kSparse || c < n_cols)) ? c : -1; // (sparse: any c >= 0 is a key)
            } else {
                lab = in ? v : K;
            }
        }
        s_lab[p] = lab;
        if (!kVotes)
            for (int i = p; i < kAssocTable; i += kAssocThreads)
                s_key[i] = kAssocEmpty, s_val[i] = 0ull;
    }
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const u32 wave = uniform(threadIdx.x >> 6);
    const Header *hb = headers + tile_offsets[tile];
    // the batch of leader sums: lane i holds the i-th (destination, value) this wave has produced, n_out is wave-uniform.  votes: the
    // destination is an element of V and the flush ONE 8-byte global atomic instruction; overlap: it is the element's offset in O,
    // row * ld + col, and the flush one pass of `combine` for up to 64 keys instead of a serial LDS round trip per leader
    u64 out_at = 0ull;
    u32 out_v = 0;
    u32 n_out = 0;
    auto stage = [&](u64 at, u32 v) {
        if ((u32)lane == n_out)
            out_at = at, out_v = v;
        ++n_out;
    };
    // overlap: q into the workgroup's table for every lane with act set; a fixed number of probes, then O itself
    auto combine = [&](bool act, u64 key, u32 q) { // key: the element's offset in O
        act = act && q != 0u;
        u32 slot = (((u32)key * 0x9E3779B1u) ^ ((u32)(key >> 32) * 0x85EBCA6Bu)) >> 23; // 9 bits = kAssocTable
        for (int p = 0; p < kAssocProbes; ++p) {
            if (__builtin_amdgcn_ballot_w64(act) == 0ull)
                break;
            if (act) {
                const u64 prev = atomicCAS(&s_key[slot], kAssocEmpty, key);
                if (prev == kAssocEmpty || prev == key) {
                    atomicAdd(&s_val[slot], (u64)q);
                    act = false;
                } else {
                    slot = (slot + 1u) & (u32)(kAssocTable - 1);
                }
            }
        }
        if (act)
            atomicAdd(out + key, (u64)q);
    };
    // sparse: v to the slot of `row` whose key is `key` (the first empty one becomes it), else to spill[row]; key kAssocTotal: to
    // total[row].  Slots in index order, one probe per trip, the trip count wave-uniform
    auto sparse_add = [&](bool act, u32 row, int key, u32 v) {
        act = act && v != 0u;
        if (act && key == kAssocTotal) {
            atomicAdd(SP.total + row, (u64)v);
            act = false;
        }
        int32_t *kp = SP.keys + (int64_t)row * SP.ldk;
        u64 *vp = SP.vals + (int64_t)row * SP.ldv;
        for (int s = 0; s < SP.slots; ++s) {
            if (__builtin_amdgcn_ballot_w64(act) == 0ull)
                break;
            if (act) {
                int cur = __hip_atomic_load(kp + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (cur == -1) {
                    cur = atomicCAS(kp + s, -1, key);
                    cur = cur == -1 ? key : cur; // ours now; or somebody else's key, which stays
                }
                if (cur == key) {
                    atomicAdd(vp + s, (u64)v);
                    act = false;
                }
            }
        }
        if (act)
            atomicAdd(SP.spill + row, (u64)v);
    };
    auto flush = [&]() {
        if (kSparse) {
            sparse_add((u32)lane < n_out, (u32)(out_at >> 32), (int)(u32)out_at, out_v);
        } else if (kVotes) {
            if ((u32)lane < n_out && out_v != 0u)
                atomicAdd(out + out_at, (u64)out_v);
        } else {
            combine((u32)lane < n_out, out_at, out_v);
        }
        n_out = 0;
    };
    static_assert(kAssocTable == 512, "the slot hash keeps 9 bits");

    for (u32 h = wave; h < nh; h += kAssocThreads / 64) {
        if (n_out > 64u - kAssocRounds - (kSparse ? 1u : 0u)) // a record stages at most kAssocRounds sums (sparse: and its total)
            flush();
        const Header *hp = hb + h;
        const u32 gid = uniform(hp->gid), w0 = uniform(hp->woff[0]), w2 = uniform(hp->woff[2]);
        const u32 counts = uniform(hp->counts);
        const u32 n01 = (counts & 0xFFu) + ((counts >> 8) & 0xFFu);
        const u32 n = n01 + ((counts >> 16) & 0xFFu) + (counts >> 24);
        u64 base = (u64)gid * (u64)ld; // votes: the Gaussian's row; overlap: the record's column, 0 = unassigned
        if (!kVotes) {
            const int g = (int)uniform((u32)aux[gid]);
            base = (g >= 0 && g <= n_cols - 2) ? (u64)(g + 1) : 0ull;
        }
        if (kSparse)
            base = (u64)gid << 32; // a staged entry is (row, key)
        const u64 step = kVotes ? 1ull : (u64)ld; // a staged value k lies at base + k * step

        int lab[kAssocSlots];
        u32 q[kAssocSlots];
        bool pend[kAssocSlots];
#pragma unroll
        for (int k = 0; k < kAssocSlots; ++k) {
            lab[k] = -1, q[k] = 0u;
            const u32 i = (u32)(k * 64 + lane);
            if ((u32)(k * 64) < n && i < n) {
                const WPair e = wpool[i < n01 ? w0 + i : w2 + (i - n01)];
                q[k] = assoc_quantize(e.w);
                lab[k] = s_lab[e.pix & 255u]; // (a stored entry's pixel is < 256; the padding is not read)
            }
            pend[k] = lab[k] >= 0 && q[k] != 0u;
        }
        if (kSparse && SP.total) // every entry counts here, whatever its label: the exact denominator of a label field
            stage(base | (u64)(u32)kAssocTotal, wave_sum_u32(q[0] + q[1] + q[2] + q[3]));

        for (int r = 0; r < kAssocRounds; ++r) {
            u64 any = 0ull;
#pragma unroll
            for (int k = 0; k < kAssocSlots; ++k)
                any |= __builtin_amdgcn_ballot_w64(pend[k]);
            if (any == 0ull)
                break;
            int cand = -1; // this lane's first pending key
#pragma unroll
            for (int k = kAssocSlots - 1; k >= 0; --k)
                cand = pend[k] ? lab[k] : cand;
            const int key = __builtin_amdgcn_readlane(cand, (int)__builtin_ctzll(any));
            u32 s = 0u;
#pragma unroll
            for (int k = 0; k < kAssocSlots; ++k) {
                const bool m = pend[k] && lab[k] == key;
                s += m ? q[k] : 0u;
                pend[k] = pend[k] && !m;
            }
            stage(base + (u64)key * step, wave_sum_u32(s));
        }
        // more distinct keys than leader rounds: every entry still pending adds its own value (one pass per slot of four)
#pragma unroll
        for (int k = 0; k < kAssocSlots; ++k) {
            if (__builtin_amdgcn_ballot_w64(pend[k]) == 0ull)
                continue;
            const u64 at = base + (u64)(pend[k] ? lab[k] : 0) * step;
            if (kSparse) {
                sparse_add(pend[k], gid, lab[k], q[k]);
            } else if (kVotes) {
                if (pend[k])
                    atomicAdd(out + at, (u64)q[k]);
            } else {
                combine(pend[k], at, q[k]);
            }
        }
    }
    flush();
    if (kVotes)
        return;
    __syncthreads();
    for (int i = threadIdx.x; i < kAssocTable; i += kAssocThreads) {
        const u64 key = s_key[i], v = s_val[i];
        if (key != kAssocEmpty && v != 0ull)
            atomicAdd(out + key, v);
    }
}

template <typename T, bool kVotes>
__global__ __launch_bounds__(kAssocThreads) void k_label_assoc(
    ViewDev V, const u32 *__restrict__ tile_order, const u32 *__restrict__ tile_offsets, const u32 *__restrict__ hdr_count,
    const Header *__restrict__ headers, const WPair *__restrict__ wpool, const T *__restrict__ labels, int64_t ls_y, int64_t ls_x,
    const int32_t *__restrict__ ymap, const int32_t *__restrict__ xmap, int K, const int32_t *__restrict__ aux, int n_cols,
    u64 *__restrict__ out, int64_t ld, Counters *__restrict__ ctr)
{
    assoc_walk<T, kVotes ? kAssocVotes : kAssocOverlap>(V, tile_order, tile_offsets, hdr_count, headers, wpool, labels, ls_y, ls_x, ymap,
                                                        xmap, K, aux, n_cols, out, ld, ctr, SparseDev{});
}

template <typename T>
__global__ __launch_bounds__(kAssocThreads) void k_label_votes_sparse(
    ViewDev V, const u32 *__restrict__ tile_order, const u32 *__restrict__ tile_offsets, const u32 *__restrict__ hdr_count,
    const Header *__restrict__ headers, const WPair *__restrict__ wpool, const T *__restrict__ labels, int64_t ls_y, int64_t ls_x,
    const int32_t *__restrict__ ymap, const int32_t *__restrict__ xmap, int K, const int32_t *__restrict__ remap, SparseDev SP,
    Counters *__restrict__ ctr)
{
    assoc_walk<T, kAssocSparse>(V, tile_order, tile_offsets, hdr_count, headers, wpool, labels, ls_y, ls_x, ymap, xmap, K, remap, 0,
                                nullptr, 0, ctr, SP);
}

template <typename T, int kMode>
static void launch_assoc_t(const Ws &W, const ViewDev &V, const void *labels, int64_t ls_y, int64_t ls_x, const int32_t *ymap,
                           const int32_t *xmap, int K, const int32_t *aux, int n_cols, int64_t *out, int64_t ld,
                           const SparseDev &SP, hipStream_t s)
{
    const int n_tiles = V.tile_w * V.tile_h;
    if (kMode == kAssocSparse)
        hipLaunchKernelGGL((k_label_votes_sparse<T>), dim3(n_tiles), dim3(kAssocThreads), 0, s, V, W.tile_order, W.tile_offsets,
                           W.hdr_count, W.headers, W.wpool, static_cast<const T *>(labels), ls_y, ls_x, ymap, xmap, K, aux, SP,
                           W.counters);
    else
        hipLaunchKernelGGL((k_label_assoc<T, kMode == kAssocVotes>), dim3(n_tiles), dim3(kAssocThreads), 0, s, V, W.tile_order,
                           W.tile_offsets, W.hdr_count, W.headers, W.wpool, static_cast<const T *>(labels), ls_y, ls_x, ymap, xmap, K,
                           aux, n_cols, reinterpret_cast<u64 *>(out), ld, W.counters);
}

template <int kMode>
static void launch_assoc(const Ws &W, const ViewDev &V, const void *labels, int label_type, int64_t ls_y, int64_t ls_x,
                         const int32_t *ymap, const int32_t *xmap, int K, const int32_t *aux, int n_cols, int64_t *out, int64_t ld,
                         const SparseDev &SP, hipStream_t s)
{
    if (label_type == GWBP_LABEL_U8)
        launch_assoc_t<uint8_t, kMode>(W, V, labels, ls_y, ls_x, ymap, xmap, K, aux, n_cols, out, ld, SP, s);
    else if (label_type == GWBP_LABEL_I16)
        launch_assoc_t<int16_t, kMode>(W, V, labels, ls_y, ls_x, ymap, xmap, K, aux, n_cols, out, ld, SP, s);
    else
        launch_assoc_t<int32_t, kMode>(W, V, labels, ls_y, ls_x, ymap, xmap, K, aux, n_cols, out, ld, SP, s);
}

int launch_label_overlap(const Layout &L, const Ws &W, const ViewDev &V, const void *labels, int label_type, int64_t ls_y,
                         int64_t ls_x, const int32_t *ymap, const int32_t *xmap, int K, const int32_t *group, int n_cols, int64_t *O,
                         int64_t ldo, hipStream_t s)
{
    (void)L;
    launch_assoc<kAssocOverlap>(W, V, labels, label_type, ls_y, ls_x, ymap, xmap, K, group, n_cols, O, ldo, SparseDev{}, s);
    return check_hip(hipGetLastError(), "label_overlap launch");
}

int launch_label_votes(const Layout &L, const Ws &W, const ViewDev &V, const void *labels, int label_type, int64_t ls_y,
                       int64_t ls_x, const int32_t *ymap, const int32_t *xmap, int K, const int32_t *remap, int n_cols, int64_t *Vt,
                       int64_t ldv, hipStream_t s)
{
    (void)L;
    launch_assoc<kAssocVotes>(W, V, labels, label_type, ls_y, ls_x, ymap, xmap, K, remap, n_cols, Vt, ldv, SparseDev{}, s);
    return check_hip(hipGetLastError(), "label_votes launch");
}

int launch_label_votes_sparse(const Layout &L, const Ws &W, const ViewDev &V, const void *labels, int label_type, int64_t ls_y,
                              int64_t ls_x, const int32_t *ymap, const int32_t *xmap, int K, const int32_t *remap, int slots,
                              int32_t *keys, int64_t ld_keys, int64_t *vals, int64_t ld_vals, int64_t *spill, int64_t *total,
                              hipStream_t s)
{
    (void)L;
    SparseDev SP;
    SP.keys = keys;
    SP.vals = reinterpret_cast<u64 *>(vals);
    SP.spill = reinterpret_cast<u64 *>(spill);
    SP.total = reinterpret_cast<u64 *>(total);
    SP.ldk = ld_keys, SP.ldv = ld_vals, SP.slots = slots;
    launch_assoc<kAssocSparse>(W, V, labels, label_type, ls_y, ls_x, ymap, xmap, K, remap, 0, nullptr, 0, SP, s);
    return check_hip(hipGetLastError(), "label_votes_sparse launch");
}

} // namespace gwbp
