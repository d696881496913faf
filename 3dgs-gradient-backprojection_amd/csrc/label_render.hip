// label_render.hip -- per-Gaussian labels rendered to 2-D class maps and scored against a ground-truth label map.
//
// The mirror image of k_scatter_labels (label.hip): that kernel lifts a label map onto the Gaussians without a one-hot map, this
// one renders labels[N] without a one-hot [N, K] table.  The reference (affordance_transfer/demo_affordance_transfer.py:1445-1611,
// evaluate_results) renders one 3-channel 0/1 indicator table per class and view, copies each [H, W, 3] image to the host,
// thresholds it there (torch_to_cv: clamp to [0, 1], x 255, uint8; then > 64) and counts against the ground truth in numpy.
// k_render_labels blends a view ONCE: the payload of a record is one int32, the K class sums of a pixel are a lane-owned LDS
// column, and threshold, comparison and counts happen in the kernel's epilogue -- no image has to leave the device.
//
// k_render_labels is a tile rasteriser in the shape of k_render_px (render.hip): workgroup = 16x16 tile, thread = pixel, records
// staged in LDS per batch of 256, the blend step of px_blend.h (alpha and T bit-identical).  It needs project + bin_sort only.
//   maps[p, k]  = sum over the contributing records of label k, front to back, of w: bin = bin + w.  That is the k_render_px
//                 render of the one-hot table bit for bit (fma(w, 1, a) = a + w, fma(w, 0, a) = a for the finite w of a valid
//                 record), without its K - 1 idle FMAs per record.
//   argmax[p]   = the class of the largest sum, the lowest index among equals; -1 where no class has a sum above 0 or the
//                 largest lies below min_opacity.
//   counts[k]   = {intersection, predicted, ground truth} pixels of class k, added to what is there: ballots and popcounts per
//                 wave into LDS integers, then one 64-bit integer atomic per non-zero counter and workgroup.  Integer sums do not
//                 depend on their order: the counts are bit-reproducible.  The kernel has no float atomic.
// One launch takes up to kLabelChunk classes; launch_render_labels walks wider tables chunk by chunk (class sums are independent,
// so this is exact): a chunk sees labels - base, ignores what falls outside [0, chunk), and carries the running (sum, class)
// pair of the argmax through `best` / `argmax`.
#include "gwbp_dev.h"
#include "px_blend.h"

namespace gwbp {

constexpr int kLabelChunk = 64; // classes per launch: 64 KB of class sums per workgroup, two workgroups per CU

namespace {

struct LabelOut {
    float *maps;         // [H, W, K] or nullptr
    float *alphas;       // [H, W] or nullptr
    int32_t *argmax;     // [H, W] or nullptr
    float *best;         // [H, W] or nullptr: the largest class sum (the carry of the argmax between chunks)
    const int32_t *gt;   // [H, W]; read only with counts
    u64 *counts;         // [K, 3] or nullptr
};

// x -> label relative to the chunk, -1 outside it (unsigned: no label can wrap into [0, n): base + n <= 2^31)
__device__ __forceinline__ int chunk_label(int32_t x, int base, int n)
{
    const u32 rel = (u32)x - (u32)base;
    return rel < (u32)n ? (int)rel : -1;
}

// K: classes of the table (the pixel stride of maps); [base, base + kc): the classes of this launch; first / last: the chunk's
// place in the walk (first: the argmax pair starts at (0, -1); last: min_opacity is applied); thr = (float)(cut + 1).
__global__ __launch_bounds__(256) void k_render_labels(ViewDev V, const u32 *__restrict__ tile_offsets, const u32 *__restrict__ vals,
                                                       const G2D *__restrict__ g2d, const int32_t *__restrict__ labels, int K,
                                                       int base, int kc, int first, int last, float thr, float min_opacity,
                                                       LabelOut O)
{
    __shared__ float4 s_a[256]; // mx, my, opac, ln(255 opac) + margin
    __shared__ float4 s_b[256]; // ca, cb, cc, -
    __shared__ int s_lab[256];  // the record's class inside the chunk, -1: none
    __shared__ u32 s_cnt[3 * kLabelChunk];
    extern __shared__ float s_bin[]; // [kc][256]: thread t owns column t (address k * 256 + t: conflict-free)
    const int tid = threadIdx.x;
    const int tile = blockIdx.x;
    const int tx = tile % V.tile_w, ty = tile / V.tile_w;
    const int lane = tid & 63;
    const int wave = (int)uniform(threadIdx.x >> 6);
    const int ix = tx * kTile + (lane & 15), iy = ty * kTile + wave * 4 + (lane >> 4);
    const bool inside = ix < V.W && iy < V.H;
    const float px = (float)ix + 0.5f, py = (float)iy + 0.5f;
    const u32 beg = tile_offsets[tile], end = tile_offsets[tile + 1];
    for (int k = 0; k < kc; ++k)
        s_bin[k * 256 + tid] = 0.f;
    if (tid < 3 * kLabelChunk)
        s_cnt[tid] = 0u;
    float T = 1.0f;
    bool done = !inside;
    // the column entry of the class taken last stays in a register: neighbouring records mostly share their label, and
    // bin = bin + w is the same sum wherever bin lives
    int cur = -1;
    float run = 0.f;
    for (u32 batch = beg; batch < end; batch += 256) {
        if (__syncthreads_count(done) == 256)
            break;
        const u32 bn = min(256u, end - batch);
        if (threadIdx.x < bn) {
            const u32 gid = vals[batch + threadIdx.x];
            const float4 *gp = reinterpret_cast<const float4 *>(g2d + gid);
            s_a[threadIdx.x] = px_stage(gp[0]);
            s_b[threadIdx.x] = gp[1];
            s_lab[threadIdx.x] = chunk_label(labels[gid], base, kc);
        }
        __syncthreads();
        for (u32 j = 0; j < bn; ++j) {
            if (__ballot(!done) == 0ull)
                break;
            const float4 a = s_a[j], b = s_b[j];
            const float sigma = px_sigma(a, b, px, py);
            if (px_quarter_outside(done, sigma, a.w))
                continue;
            float w;
            const bool valid = px_step(sigma, a.z, T, done, w);
            if (px_nobody(valid))
                continue;
            const int lab = (int)uniform((u32)s_lab[j]);
            if (lab < 0)
                continue; // contributes to alpha, to no class
            if (lab != cur) { // wave-uniform
                if (cur >= 0)
                    s_bin[cur * 256 + tid] = run;
                cur = lab;
                run = s_bin[lab * 256 + tid];
            }
            run = valid ? run + w : run;
        }
    }
    if (cur >= 0)
        s_bin[cur * 256 + tid] = run;
    __syncthreads(); // s_cnt is zero in every wave's eyes (the columns are private)

    const size_t p = (size_t)iy * V.W + ix;
    const bool count = O.counts != nullptr;
    const int gtv = (count && inside) ? chunk_label(O.gt[p], base, kc) : -1;
    float best = 0.f;
    int best_k = -1;
    if (!first && O.best && inside) { // the pair the chunks before this one left
        best = O.best[p];
        best_k = O.argmax ? O.argmax[p] : -1;
    }
    float *mp = O.maps ? O.maps + p * (size_t)K + base : nullptr;
    for (int k = 0; k < kc; ++k) {
        const float x = s_bin[k * 256 + tid];
        if (mp && inside)
            mp[k] = x;
        if (x > best) { // strictly: the lowest index wins a tie, and a zero sum never wins
            best = x;
            best_k = base + k;
        }
        if (count) { // uniform
            // torch_to_cv(...) > cut: clamp to [0, 1], ONE fp32 multiply by 255 (the file is compiled without contraction),
            // truncation to uint8; trunc(v) > cut <=> v >= cut + 1
            const float v = __builtin_fminf(__builtin_fmaxf(x, 0.f), 1.0f) * 255.0f;
            const u64 pred = __ballot(inside && v >= thr);
            const u64 truth = __ballot(gtv == k);
            if (lane == 0) {
                const u32 n_i = (u32)__popcll(pred & truth), n_p = (u32)__popcll(pred), n_g = (u32)__popcll(truth);
                if (n_i)
                    atomicAdd(&s_cnt[3 * k], n_i);
                if (n_p)
                    atomicAdd(&s_cnt[3 * k + 1], n_p);
                if (n_g)
                    atomicAdd(&s_cnt[3 * k + 2], n_g);
            }
        }
    }
    if (inside) {
        if (O.alphas)
            O.alphas[p] = 1.0f - T;
        if (O.argmax)
            O.argmax[p] = (last && best < min_opacity) ? -1 : best_k;
        if (O.best)
            O.best[p] = best;
    }
    if (count) {
        __syncthreads();
        if (tid < 3 * kc && s_cnt[tid] != 0u)
            atomicAdd(O.counts + (size_t)3 * base + tid, (u64)s_cnt[tid]);
    }
}

} // namespace

int launch_render_labels(const Ws &W, const ViewDev &V, const int32_t *labels, int K, float *maps, float *alphas, int32_t *argmax,
                         float *best, float min_opacity, const int32_t *gt, int cut, u64 *counts, hipStream_t s)
{
    const int n_tiles = V.tile_w * V.tile_h;
    const int fin = sort_passes(n_tiles) & 1;
    // static (staging, counters) + dynamic (class sums) LDS pass the 64 KB a kernel gets unasked from 54 classes on
    int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(k_render_labels), kLabelChunk * 256 * (int)sizeof(float));
    if (rc)
        return rc;
    for (int base = 0; base < K; base += kLabelChunk) {
        const int kc = K - base < kLabelChunk ? K - base : kLabelChunk;
        // the alpha map does not depend on the classes: the first chunk writes it
        const LabelOut O{maps, base == 0 ? alphas : nullptr, argmax, best, gt, counts};
        hipLaunchKernelGGL(k_render_labels, dim3(n_tiles), dim3(256), (size_t)kc * 256 * sizeof(float), s, V, W.tile_offsets,
                           W.vals[fin], W.g2d, labels, K, base, kc, base == 0, base + kc == K, (float)(cut + 1), min_opacity, O);
        if ((rc = check_hip(hipGetLastError(), "render_labels launch")))
            return rc;
    }
    return GWBP_OK;
}

} // namespace gwbp
