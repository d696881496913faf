// gwbp_dev.h -- internal declarations shared by the HIP translation units of libgwbp.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/gwbp.h"

namespace gwbp {

typedef unsigned long long u64;
typedef unsigned int u32;

// ---- constants of the arithmetic contract (gsplat 1.4.0 semantics) -------------
constexpr float kAlphaMin = 0x1.010102p-8f;    // 1/255
constexpr float kAlphaMax = 0x1.ff7ceep-1f;    // 0.999
constexpr float kTMin = 0x1.a36e2ep-14f;       // 1e-4
constexpr float kRadiusFloor = 0x1.47ae14p-7f; // 0.01
constexpr float kClampMargin = 0x1.333334p-2f; // 0.3 (x/z clamp margin in tan_fov units)

constexpr int kTile = GWBP_TILE;     // 16 x 16 pixels
constexpr int kTilePix = 256;
constexpr int kPage = 1024;          // weight-pool page (pairs) grabbed per (tile, wave) stream
constexpr int kQueues = 8;           // scatter work queues, one per XCD class (blockIdx % 8), 64 B apart, after the shard heads
constexpr int kShards = 32;          // independently counted regions of the weight pool (one head word per 64-B line)
// Words of a shard's 64-B line (blend.hip): the head, then what the running blend has counted of the tiles of that shard -- its
// n_headers and (8-B aligned) n_pairs -- until the blend's end moves them into Counters and zeroes them.  Line 0 also holds the
// leaver counts of the blends that end in their own last wave (fused, token) and the split encoder's tile counter.  All of them
// are zero between two blends.
constexpr int kShardHead = 0, kShardHeaders = 1, kShardPairs = 2; // kShardPairs: a u64 (words 2 and 3)
constexpr int kBlendLeavers = 4, kPcTileCounter = 5, kPcProducerLeavers = 6; // in line 0
constexpr int kListPad = 8;          // every record's entry list is padded to a multiple of kListPad entries (kHalves: each half's)
constexpr unsigned kPadPix = 640;    // "pixel" of a padding entry {0, kPadPix}: its slab row lies beyond the 160 KB an LDS allocation
                                     // can have in the 256-channel kernel (1 KB rows), where an out-of-range read returns 0; every
                                     // other consumer masks the padding by the quarters' counts
constexpr int kSortItems = 4096;     // keys per sort block (256 threads x 16)
constexpr int kScanBlock = 256;      // Gaussians per project/emit block
constexpr int kMaxPasses = 4;        // 8-bit passes per sort level (32-bit keys)
// the sort's small tables, cleared with the counters by gwbp_project's memset: digit totals [2 levels][kMaxPasses][256] (one
// k_hist_all per level fills a level's tables from one read of the keys), then one block ticket per (level, pass)
constexpr int kSweepTickets = 2 * kMaxPasses * 256;
constexpr int kSweepWords = kSweepTickets + 2 * kMaxPasses;

// ---- device-resident tables -------------------------------------------------------------------------------
// Projected Gaussian, 32 B, read by the blend kernel with two 16-B loads.
struct __attribute__((aligned(16))) G2D {
    float mx, my, opac, depth;
    float ca, cb, cc;
    int radius; // 0 = culled
};

// One entry of the sparse weight store: w = alpha * T of one (Gaussian, pixel) pair and the pixel's index inside its
// 16x16 tile (row-major, 0..255).  8 B so that eight entries are one s_load_dwordx16 and {w, pix} is an aligned SGPR pair.
struct __attribute__((aligned(8))) WPair {
    float w;
    u32 pix;
};

// One per (Gaussian, tile) pair that contributes at least one weight.  mask[q] bit l <=> pixel q*64+l of the tile
// (row-major 16x16) has a weight; the popc(mask[q]) entries of quarter q are contiguous at wpool[woff[q]..] in
// ascending pixel order.  INVARIANTS the scatter kernels rely on: quarters 0 | 1 are back to back (woff[1] = woff[0] + cnt0) and
// so are quarters 2 | 3; woff[0] % kListPad == 0; the record ends with {0, kPadPix} entries up to the next multiple of kListPad.
// A store blended for the 256-channel kernel (k_blend<kHalves>) additionally pads the FIRST half: woff[2] % kListPad == 0 with
// {0, kPadPix} entries between the halves (k_scatter_wide fetches a half's entries eight at a time); otherwise woff[2] =
// woff[1] + cnt1.  A reader of the whole record as one run (k_scatter_full) takes woff[3] + cnt3 - woff[0] entries and drops
// those with pix >= 256.
// counts = cnt0 | cnt1 << 8 | cnt2 << 16 | cnt3 << 24 (cnt <= 64).
struct __attribute__((aligned(64))) Header {
    u32 gid;
    u32 woff[4];
    u32 counts;
    u32 wsum; // float bits: sum of the record's weights = the record's share of d[gid] (k_accum_d)
    u32 carry_row; // k_blend<kHalves>: the record's rank among its tile's records that have entries in both halves (its carry row
                   // in k_scatter_wide), 0xFFFFFFFF for a record that lies in one half; unused otherwise
    u64 mask[4];
};
static_assert(sizeof(Header) == 64, "header is one 64-B line");

constexpr int kCarryRows = 1024; // carry rows per scatter workgroup; a tile's records beyond it are flushed per half
constexpr int kCarryWgs = 256;   // scatter workgroups that own a carry slice (persistent grid: one per CU)

// Mirrors gwbp_stats (include/gwbp.h) field for field.
struct Counters {
    u64 n_pairs;
    u32 n_isect;
    u32 n_visible;
    u32 n_headers;
    u32 pool_head;
    u32 overflow;
    u32 blend_kind; // gwbp_stats::reserved: kBlendHalves once k_blend<kHalves> has written THIS view's weight sums
};
constexpr u32 kBlendHalves = 1u;
constexpr u32 kBlendFused = 2u; // gwbp_blend_scatter: the view was blended AND scattered, its weight store is empty
constexpr u32 kBlendToken = 3u; // gwbp_blend_tokens: the workspace holds per-(Gaussian, tile) token-quadrant weight sums, no store
constexpr u32 kOverflowMismatch = 4u; // gwbp_stats::overflow bit 2, see include/gwbp.h
constexpr u32 kOverflowRingStall = 16u; // bit 4: a wave of the producer / consumer kernel gave up waiting on its LDS ring (internal error)
constexpr u32 kOverflowTokenGeometry = 8u; // bit 3: gwbp_blend_tokens met a tile that spans more than 2 x 2 tokens
static_assert(sizeof(Counters) == sizeof(gwbp_stats), "Counters must mirror gwbp_stats");

struct Layout {
    size_t total;
    size_t counters, shards, sweep, g2d, rect, touched, blocksums, dkeys[2], dvals[2], keys[2], vals[2], hist, digit_total, tile_offsets, tile_order, hdr_count,
        headers, carry, wpool;
    int64_t n, isect_cap, pair_cap;
    int max_tiles, n_scan_blocks, n_sort_blocks, scatter_wgs, flags;
};

struct Ws {
    Counters *counters;
    u32 *shards; // kShards head words, 16 u32 apart
    u32 *sweep;  // kSweepWords: digit totals of every sort pass + block tickets (zero between gwbp_bin_sort calls)
    G2D *g2d;
    uint2 *rect; // x = xmin | xmax<<16, y = ymin | ymax<<16
    u32 *touched;
    u32 *blocksums;
    u32 *dkeys[2], *dvals[2]; // depth sort of the Gaussians: key = depth bits (0xFFFFFFFF if culled), value = index
    u32 *keys[2];             // intersection sort: key = tile id
    u32 *vals[2];             //                    value = Gaussian index
    u32 *hist;
    u32 *digit_total;
    u32 *tile_offsets;
    u32 *tile_order; // tiles by descending list length (heavy tiles start first in k_blend)
    u32 *hdr_count;
    Header *headers;
    float *carry;        // kCarryWgs x kCarryRows x 256 floats
    WPair *wpool;
};

int make_layout(const gwbp_caps *caps, Layout *L);
int bind_workspace(const gwbp_caps *caps, void *ws, size_t bytes, Layout *L, Ws *W);
int set_error(int code, const char *fmt, ...);
int check_hip(hipError_t e, const char *what);
// Per-device facts, cached per device ORDINAL (a process may drive several GPUs): CU count of the current device, and the largest
// dynamic-LDS limit each kernel has been given on the current device (raised when a kernel is new there or asks for more).
int device_cus(int *n_cu);
int ensure_dynamic_lds(const void *func, int bytes);
// workgroups of per_block items for n of them, or GWBP_EINVAL beyond what a grid's x dimension takes
inline int grid_of(const char *what, int64_t n, unsigned *grid, int per_block)
{
    const int64_t g = (n + per_block - 1) / per_block;
    if (g > 0x7FFFFFFF)
        return set_error(GWBP_EINVAL, "%s: %lld items need more than 2^31 - 1 workgroups", what, (long long)n);
    *grid = (unsigned)g;
    return GWBP_OK;
}
// Profiling / ablation knobs (GWBP_ABLATE, GWBP_ABLATE_BLEND, GWBP_BLEND_LDS): an environment variable is read only by a
// library built with -DGWBP_PROFILE (make PROFILE=1 -> libgwbp_profile.so); the product library always gets 0.
int profile_knob(const char *name);

struct ViewDev { // per-launch copy of gwbp_view (kernel argument, 128 B)
    float R[9];
    float t[3];
    float fx, fy, cx, cy;
    int W, H, tile_w, tile_h;
    float near_plane, far_plane, eps2d, radius_clip;
};
int make_view(const gwbp_view *v, const gwbp_caps *caps, ViewDev *out);

// 8-bit passes of the tile-id sort of the intersections (the depth order comes from the Gaussian pre-sort)
inline int sort_passes(int n_tiles)
{
    int tile_bits = 1;
    while ((1 << tile_bits) < n_tiles)
        ++tile_bits;
    return (tile_bits + 7) / 8;
}

// A finished field's element type (GWBP_MAP_*) on the host side of a launcher: the bytes of an element, and whether rows at p with a
// stride of ld ELEMENTS may take load4t's vector path (16-B loads of fp32 rows, 8-B loads of half rows).
inline size_t field_elem_bytes(int mt) { return mt == GWBP_MAP_F32 ? 4 : 2; }
inline bool field_rows_vec(const void *p, int64_t ld, int mt)
{
    return !(reinterpret_cast<uintptr_t>(p) & (mt == GWBP_MAP_F32 ? 15u : 7u)) && !(ld & 3);
}

// stage launchers (one per .hip file)
int launch_project(const Layout &L, const Ws &W, const ViewDev &V, const float *means, const float *quats,
                   const float *scales, const float *opac, int32_t *radii, float *means2d, float *depths,
                   float *conics, hipStream_t s, int camera_model = GWBP_CAMERA_PINHOLE,
                   int rasterize_mode = GWBP_RASTERIZE_CLASSIC, float *compensations = nullptr);
int launch_emit(const Layout &L, const Ws &W, const ViewDev &V, const u32 *order, hipStream_t s);
int launch_emit_scanned(const Layout &L, const Ws &W, const ViewDev &V, const u32 *order, hipStream_t s);
int launch_bin_sort(const Layout &L, const Ws &W, const ViewDev &V, int64_t *isect_ids, int32_t *flatten_ids,
                    int32_t *tile_offsets, hipStream_t s);
struct FeatMap;
// Per-pixel weight map of the gwbp_*_ex entry points (a validated gwbp_pixel_weights): c(x, y) = data[y * ws_y + x * ws_x], strides
// in elements, element type dtype (GWBP_PIXW_*).
struct PixW {
    const void *data;
    int64_t ws_y, ws_x;
    int dtype;
};
// M != nullptr: the fused small-D form (gwbp_blend_scatter): F[gid, :D] and d are accumulated by the blend itself.
// pw != nullptr: every blend form weighted by the map (what it adds or stores is w c(p)).
// rgb != nullptr (storing and token blends only): the RGB composite of gwbp_blend_*_rgb, image[p] = sum_g alpha T colors[g].
struct RgbOut {
    const float *colors; // [N, 3]
    float *image;        // [H, W, 3]
};
int launch_blend(const Layout &L, const Ws &W, const ViewDev &V, float *alphas, float *d, float scale_d, hipStream_t s,
                 const FeatMap *M = nullptr, int D = 0, float scale_f = 1.0f, float *F = nullptr, const PixW *pw = nullptr,
                 const RgbOut *rgb = nullptr);
// token-space path of a nearest-upsampled low-resolution map (blend.hip: k_blend<kToken>; token.hip)
int launch_blend_tokens(const Layout &L, const Ws &W, const ViewDev &V, float *alphas, const int32_t *ymap, const int32_t *xmap,
                        hipStream_t s, const PixW *pw = nullptr, const RgbOut *rgb = nullptr);
int launch_zero_omega(const Layout &L, const Ws &W, hipStream_t s);
int launch_token_apply(const Layout &L, const Ws &W, const ViewDev &V, const float *tokens, int64_t ts_y, int64_t ts_x, int D,
                       const int32_t *ymap, const int32_t *xmap, float scale_f, float scale_d, float *F, float *d, hipStream_t s);
// A 2-D feature map as the scatter kernels address it: feats[row(y)*fs_y + col(x)*fs_x + c*fs_c] (strides in floats).
// ymap/xmap (device, optional) send an output pixel to the row/column of a lower-resolution map: the
// F.interpolate(mode="nearest") of backproject.py:244-248 without materialising the upsampled map.  With ly/lx as well
// the map is sampled BILINEARLY (backproject.py:110-112, align_corners=False): ymap/xmap hold the lower texel, ly/lx
// the weight of the upper one, lr_h/lr_w clamp the upper texel; ATen's operation order is kept.
struct FeatMap {
    const float *p;
    int64_t fs_y, fs_x, fs_c;
    const int32_t *ymap, *xmap;
    const float *ly, *lx;
    int32_t lr_h, lr_w;
    // gwbp_scatter_encoded (small-D kernel only): the map has enc_k channels per pixel and is multiplied by
    // enc[enc_k, D] while the tile's slab is staged (backproject_compressed.py:127 without the [H,W,D] intermediate)
    const float *enc = nullptr;
    int32_t enc_k = 0;
    __host__ __device__ __forceinline__ int64_t pixel(int iy, int ix) const
    {
        const int64_t yy = ymap ? ymap[iy] : iy, xx = xmap ? xmap[ix] : ix;
        return yy * fs_y + xx * fs_x;
    }
    __host__ __device__ __forceinline__ bool bilinear() const { return ly != nullptr; }
    // one channel of one pixel; chan = p + c * fs_c
    __device__ __forceinline__ float sample(const float *chan, int iy, int ix) const
    {
        if (!bilinear())
            return chan[pixel(iy, ix)];
        const int y0 = ymap[iy], x0 = xmap[ix];
        const int y1 = min(y0 + 1, lr_h - 1), x1 = min(x0 + 1, lr_w - 1);
        const float h1 = ly[iy], w1 = lx[ix], h0 = 1.0f - h1, w0 = 1.0f - w1;
        const float a = chan[y0 * fs_y + x0 * fs_x], b = chan[y0 * fs_y + x1 * fs_x];
        const float c = chan[y1 * fs_y + x0 * fs_x], d = chan[y1 * fs_y + x1 * fs_x];
        return h0 * (w0 * a + w1 * b) + h1 * (w0 * c + w1 * d); // UpSampleBilinear2d: same association
    }
};
// mt (GWBP_MAP_*): the element type of M.p (strides in elements); half maps take the 256- and 128-channel kernels only
int launch_scatter(const Layout &L, const Ws &W, const ViewDev &V, const FeatMap &M, int D, float scale_f,
                   float scale_d, float *F, float *d, hipStream_t s, int mt = GWBP_MAP_F32);
int launch_scatter_full(const Layout &L, const Ws &W, const ViewDev &V, const FeatMap &M, int D, float scale_f,
                        float scale_d, float *F, float *d, hipStream_t s);
int launch_accum_d(const Layout &L, const Ws &W, const ViewDev &V, float scale_d, float *d, hipStream_t s);
int launch_scatter_wide(const Layout &L, const Ws &W, const ViewDev &V, const FeatMap &M, int D, float scale_f,
                        float *F, hipStream_t s);
// the half-map instantiations (scatter_wide_half.hip, scatter_full_half.hip, token_half.hip): mt = GWBP_MAP_F16 / GWBP_MAP_BF16
int launch_scatter_wide_half(const Layout &L, const Ws &W, const ViewDev &V, const FeatMap &M, int D, float scale_f,
                             float *F, hipStream_t s, int mt);
int launch_scatter_full_half(const Layout &L, const Ws &W, const ViewDev &V, const FeatMap &M, int D, float scale_f,
                             float scale_d, float *F, float *d, hipStream_t s, int mt);
int launch_token_apply_half(const Layout &L, const Ws &W, const ViewDev &V, const void *tokens, int64_t ts_y, int64_t ts_x,
                            int D, const int32_t *ymap, const int32_t *xmap, float scale_f, float scale_d, float *F, float *d,
                            hipStream_t s, int mt);
// integer label maps (label.hip): F[g, L(p)] += scale_f * w, d[g] += scale_d * w; label_type = GWBP_LABEL_*
int launch_scatter_labels(const Layout &L, const Ws &W, const ViewDev &V, const void *labels, int label_type, int64_t ls_y,
                          int64_t ls_x, const int32_t *ymap, const int32_t *xmap, int K, float scale_f, float scale_d, float *F,
                          int64_t ldf, float *d, hipStream_t s);
// per-view votes of label maps (votes.hip): the binary vote over the weight store (k_vote_labels + k_vote_commit, seen: the caller's
// [N][ceil((K + 1) / 32)] bitset, all zero between calls) and the projection vote over the projected table (k_vote_projected)
int launch_vote_labels(const Layout &L, const Ws &W, const ViewDev &V, const void *labels, int label_type, int64_t ls_y,
                       int64_t ls_x, const int32_t *ymap, const int32_t *xmap, int K, u32 *seen, float *C, int64_t ldc, float *n,
                       hipStream_t s);
int launch_vote_projected(const Layout &L, const Ws &W, const ViewDev &V, const void *labels, int label_type, int64_t ls_y,
                          int64_t ls_x, const int32_t *ymap, const int32_t *xmap, const PixW *pw, int K, float *C, int64_t ldc,
                          float *n, hipStream_t s);
// the integer walks of the weight store behind the mask association (associate.hip), q(w) = rint(clamp(w, 0, 4) * 2^20):
// O[row(L(p)), group[g] + 1] += q (int64 [K + 1, ldo]) and V[g, remap[L(p)]] += q (int64 [N, ldv])
int launch_label_overlap(const Layout &L, const Ws &W, const ViewDev &V, const void *labels, int label_type, int64_t ls_y,
                         int64_t ls_x, const int32_t *ymap, const int32_t *xmap, int K, const int32_t *group, int n_cols, int64_t *O,
                         int64_t ldo, hipStream_t s);
int launch_label_votes(const Layout &L, const Ws &W, const ViewDev &V, const void *labels, int label_type, int64_t ls_y,
                       int64_t ls_x, const int32_t *ymap, const int32_t *xmap, int K, const int32_t *remap, int n_cols, int64_t *Vt,
                       int64_t ldv, hipStream_t s);
// the votes into per-Gaussian slot lists: keys int32 [N, ld_keys] (-1 empty), vals int64 [N, ld_vals], spill, total (or NULL) [N]
int launch_label_votes_sparse(const Layout &L, const Ws &W, const ViewDev &V, const void *labels, int label_type, int64_t ls_y,
                              int64_t ls_x, const int32_t *ymap, const int32_t *xmap, int K, const int32_t *remap, int slots,
                              int32_t *keys, int64_t ld_keys, int64_t *vals, int64_t ld_vals, int64_t *spill, int64_t *total,
                              hipStream_t s);
// mt / ot (GWBP_MAP_*): the element types of colors (row stride ldc, in elements) and of out (dense [H, W, D])
int launch_render(const Layout &L, const Ws &W, const ViewDev &V, const void *colors, int mt, int64_t ldc, int D, void *out, int ot,
                  hipStream_t s);
// the instantiations with a half table or a half output (render_wide_half.hip); the caller checks the launch
void launch_render_half(const Ws &W, const ViewDev &V, const void *colors, int mt, int64_t ldc, int D, void *out, int ot, hipStream_t s);
int launch_render_px(const Ws &W, const ViewDev &V, const void *colors, int mt, int64_t ldc, int D, float *out, float *alphas,
                     hipStream_t s);
int launch_sh_colors(int64_t N, int degree, int K, const float *means, const float *coeffs, const float *campos,
                     float *out, hipStream_t s);
// the SH colours over a coefficient row split into head [N, k_head, 3] and tail [N, k_tail, 3] (tail may be nullptr), and their backward
// (sh.hip): v_head, v_tail and v_means may each be nullptr; campos on the host
int launch_sh_eval(int64_t N, int degree, int k_head, int k_tail, const float *means, const float *head, const float *tail,
                   const float *campos, float *out, hipStream_t s);
int launch_sh_eval_bwd(int64_t N, int degree, int k_head, int k_tail, const float *means, const float *head, const float *tail,
                       const float *campos, const float *v_colors, float *v_head, float *v_tail, float *v_means, hipStream_t s);
// the same two with campos a device pointer to three floats; v_campos [3] (nullptr, or with scratch [sh_eval_backward_blocks(N), 3]):
// minus the sum of the rows' v_means values, in a fixed order
int launch_sh_eval_dev(int64_t N, int degree, int k_head, int k_tail, const float *means, const float *head, const float *tail,
                       const float *campos_dev, float *out, hipStream_t s);
int sh_eval_backward_blocks(int64_t n);
int launch_sh_eval_bwd_dev(int64_t N, int degree, int k_head, int k_tail, const float *means, const float *head, const float *tail,
                           const float *campos_dev, const float *v_colors, float *v_head, float *v_tail, float *v_means,
                           double *v_campos, double *scratch, hipStream_t s);
// backward of launch_render_px for an fp32 table (render_grad.hip): adds into v_g2d [N, 6] and, unless nullptr, v_colors [N, D]
int launch_render_px_bwd(const Ws &W, const ViewDev &V, const float *colors, int64_t ldc, int D, const float *v_out,
                         const float *v_alpha, float *v_colors, float *v_g2d, hipStream_t s);
// v_g2d alone for tables of up to 128 channels (render_grad_wide.hip): the channels enter through one dot product per pair
int launch_render_dots_bwd(const Ws &W, const ViewDev &V, const float *colors, int64_t ldc, int D, const float *v_out,
                           const float *v_alpha, float *v_g2d, hipStream_t s);
// backward of launch_project (project_grad.hip) on the records the projection of the same view left in the workspace: WRITES the
// per-Gaussian gradients (each may be nullptr) and v_viewmat [12] (nullptr, or with scratch [project_backward_blocks(n), 12])
int project_backward_blocks(int64_t n);
int launch_project_bwd(const Layout &L, const Ws &W, const ViewDev &V, int camera_model, int rasterize_mode, const float *means,
                       const float *quats, const float *scales, const float *opac, const float *v_g2d, float *v_means, float *v_quats,
                       float *v_scales, float *v_opac, double *v_viewmat, double *scratch, hipStream_t s);
// per-Gaussian labels rendered to class maps, their argmax and the counts against a ground-truth map (label_render.hip); every
// output may be nullptr; best: the largest class sum per pixel, needed beside argmax from K > 64 on (the carry between chunks)
int launch_render_labels(const Ws &W, const ViewDev &V, const int32_t *labels, int K, float *maps, float *alphas, int32_t *argmax,
                         float *best, float min_opacity, const int32_t *gt, int cut, u64 *counts, hipStream_t s);
// a field rendered from the weight store and compared with the view's map (field_compare.hip): planes [6][H][W] or nullptr, table
// [8] float64; the rows' partial sums take field_compare_scratch_bytes(tiles) of the workspace's carry slices
size_t field_compare_scratch_bytes(int n_tiles);
// (ft: the element type of feats, ldf in its elements)
int launch_field_compare(const Layout &L, const Ws &W, const ViewDev &V, const void *feats, int ft, int64_t ldf, int D, const void *map,
                         int mt, int64_t ms_y, int64_t ms_x, int lr_h, int lr_w, const int32_t *ymap, const int32_t *xmap,
                         float *planes, double *table, hipStream_t s);
// the half-field instantiations (field_compare_half.hip); cmp_map: field_compare_kernel.h's CmpMap; the caller checks the launch
void launch_field_compare_half(int ft, int mt, bool wide2, bool vec, unsigned grid, hipStream_t s, const ViewDev &V, int empty, const Ws &W,
                               const void *feats, int64_t ldf, int D, const void *cmp_map, float *planes, double *rowsums);
// decode, compare and the gradients back through the decoder of a rendered latent field (decode_loss.hip); table [8] float64; ws:
// the caller's decode_loss_workspace_bytes(d, D) bytes
size_t decode_loss_workspace_bytes(int d, int D);
int launch_decode_loss(int H, int W, int d, int D, const float *R, int64_t ldr, const float *C, int64_t ldc, const void *map, int mt,
                       int64_t ms_y, int64_t ms_x, const PixW *pw, int l2, float scale, float *GR, int64_t ldg, float *GC,
                       int64_t ldgc, double *table, void *ws, hipStream_t s);
// the photometric loss (1 - lambda) L1 + lambda (1 - SSIM) of x against y, float32 [H, W, D] with pixel strides xs / ys (ssim.hip):
// forward, reduce and -- grad != nullptr -- backward; map [H', W', D] or nullptr; table [8] float64; ws: the caller's
// image_loss_workspace_bytes(H, W, D, grad != nullptr) bytes
size_t image_loss_workspace_bytes(int H, int W, int D, int want_grad);
int launch_image_loss(int H, int W, int D, const float *x, int64_t xs, const float *y, int64_t ys, const PixW *pw, int same,
                      float lambda, float *map, float *grad, int64_t gs, double *table, void *ws, hipStream_t s);
// densification (densify.hip): the per-step statistics, the plan (kind + the exclusive scan of the rows out; ws: the caller's
// densify_plan_workspace_bytes(N) bytes; thresholds: t_grad, t_small, t_big, t_opa, log16 on the host), the children, and the relocation
// of a [N, w] table.  child / kind may be nullptr without zero_new
size_t densify_plan_workspace_bytes(int64_t n);
int launch_densify_accumulate(int64_t N, int C, const float *v, const int32_t *radii, float sx, float sy, float *grad2d, float *count,
                              hipStream_t s);
int launch_densify_plan(int64_t N, const float *grad2d, const float *count, const float *scaling, int64_t lds_, const float *opacity,
                        const float *thresholds, int prune_big, uint8_t *kind, int64_t *offsets, void *ws, hipStream_t s);
int launch_densify_emit(int64_t N, int64_t n_out, const uint8_t *kind, const int64_t *offsets, const float *means, const float *scaling,
                        const float *rotation, const float *opacity, const float *noise, float log16, int32_t *parent, uint8_t *child,
                        float *o_means, float *o_scaling, float *o_rotation, float *o_opacity, hipStream_t s);
int launch_densify_gather(int64_t N, int64_t n_out, int w, const float *table, int64_t ldt, const int32_t *parent, const uint8_t *child,
                          const uint8_t *kind, int zero_new, float *out, int64_t ldo, hipStream_t s);
// the MCMC strategy (mcmc.hip): the plan (integer weights and dead flags, their exclusive scans and the compaction of the dead; ws: the
// caller's mcmc_plan_workspace_bytes(N) bytes), the draws, the parents' new opacity and scale, the in-place move of a [N, w] table's
// dead rows, the zeroing of the parents' rows, the per-step noise, and the device's expf / logf / powf for the tests
size_t mcmc_plan_workspace_bytes(int64_t n);
int launch_mcmc_plan(int64_t N, const float *opacity, float t_opa, int add_mode, int64_t *cdf, int64_t *dead_offsets, int32_t *dead_idx,
                     void *ws, hipStream_t s);
int launch_mcmc_draw(int64_t N, int64_t M, const int64_t *cdf, const double *u, int32_t *parent, hipStream_t s);
int launch_mcmc_update(int64_t N, int64_t M, const int32_t *parent, float min_opacity, float *opacity, float *scaling, int64_t lds_,
                       int32_t *count, hipStream_t s);
int launch_mcmc_move(int64_t N, int64_t M, int w, const int32_t *parent, const int32_t *dead_idx, float *table, int64_t ldt, hipStream_t s);
int launch_mcmc_zero_rows(int64_t N, int w, const int32_t *count, float *table, int64_t ldt, hipStream_t s);
int launch_mcmc_noise(int64_t N, float *means, const float *scaling, const float *rotation, const float *opacity, const float *z,
                      float scaler, hipStream_t s);
int launch_mcmc_libm(int64_t N, int op, const float *a, const float *b, float *out, hipStream_t s);
// one Adam step of a [N, w] table in place (adam.hip, adam_math.h); visible: uint8 [N] or nullptr (every row); b1, b2 in float64: the
// launcher forms 1 - b1 and 1 - b2 there and rounds once
int launch_adam_step(int64_t N, int w, float *p, const float *g, float *m, float *v, const uint8_t *visible, float lr_over_bc1,
                     float sqrt_bc2, double b1, double b2, float eps, hipStream_t s);
// the depth losses of training (depth_loss.hip, depth_math.h): the point term and the map term, each forward (the float32 loss to a
// device scalar through per-workgroup float64 partials in ws) and backward (the upstream gradient read from the device)
size_t depth_points_workspace_bytes(int64_t M);
size_t depth_map_workspace_bytes(int H, int W);
int launch_depth_points_loss(int H, int W, int Dp, int ch, const float *render, const float *alpha, int64_t M, const float *points,
                             const float *depths, float scale, float *loss, float *per_point, double *ws, hipStream_t s);
int launch_depth_points_backward(int H, int W, int Dp, int ch, const float *render, const float *alpha, int64_t M, const float *points,
                                 const float *depths, float scale, const float *upstream, float *v_render, float *v_alpha,
                                 hipStream_t s);
int launch_depth_map_loss(int H, int W, int Dp, int ch, const float *render, const float *alpha, const float *depth,
                          const float *weights, int kind, float scale, float *loss, double *sums, double *ws, hipStream_t s);
int launch_depth_map_backward(int H, int W, int Dp, int ch, const float *render, const float *alpha, const float *depth,
                              const float *weights, int kind, float scale, const double *sums, const float *upstream, float *v_render,
                              float *v_alpha, hipStream_t s);
int launch_encode_map(const float *feats, int64_t fs_y, int64_t fs_x, int H, int W, int K, const float *enc, int n_out,
                      float *out, int workgroups, hipStream_t s);
// ot (GWBP_MAP_*): the element type of out; a half out is the fp32 result rounded once to nearest even
int launch_finalize(int64_t N, int D, const float *F, const float *d, void *out, int ot, hipStream_t s);
// inner-product k-NN search and the majority label of each row's neighbours (knn.hip)
// (here and below: mt (GWBP_MAP_*) is the element type of the FIELD operand in front of it, strides in elements; all else is fp32)
int launch_knn_search(int64_t N, int M, int D, int k, const void *Q, int mt, int64_t ldq, const float *S, int64_t lds_, int32_t *idx,
                      float *score, hipStream_t s);
int launch_knn_vote(int64_t N, int M, int k, const int32_t *idx, const int32_t *labels, int num_classes, int32_t *label_out,
                    int32_t *counts, int64_t ldc, hipStream_t s);
// exact Euclidean k-NN of 3-D points on a uniform grid and the neighbour average of a field (spatial.hip).  lo: float[3] and
// dims: int32[3] on the host
int launch_spatial_cell_keys(int64_t N, const float *P, int64_t ldp, const float *lo, float h, const int32_t *dims, int32_t *keys,
                             hipStream_t s);
int launch_spatial_build(int64_t N, const float *P, int64_t ldp, const int32_t *skeys, const int64_t *perm, int64_t n_cells,
                         float *sorted, int32_t *cell_start, hipStream_t s);
int launch_spatial_knn(const float *sorted, const int32_t *cell_start, const float *lo, float h, const int32_t *dims, int64_t Q,
                       const float *queries, int64_t ldq, const int64_t *order, int k, int32_t *idx, float *dist, hipStream_t s);
// (ot: the element type of out, ldo in ITS elements)
int launch_neighbor_mean(int64_t N, int64_t M, int D, int k, const int32_t *idx, const void *F, int mt, int64_t ldf, void *out, int ot,
                         int64_t ldo, hipStream_t s);
// radius components on the same grid (components.hip): neighbour counts within a radius, the union-find over the core points, the
// border points' nearest core neighbour, and the roots.  group / query_group / attach / visited may be nullptr
int launch_radius_count(const float *sorted, const int32_t *cell_start, const float *lo, float h, const int32_t *dims,
                        const int32_t *group, float r2, int64_t Q, const float *queries, int64_t ldq, const int64_t *order,
                        const int32_t *query_group, int cap, int32_t *count, int32_t *visited, hipStream_t s);
int launch_radius_union(int64_t N, const float *sorted, const int32_t *cell_start, const float *lo, float h, const int32_t *dims,
                        const int32_t *group, float r2, const int32_t *count, int min_points, int32_t *parent, int32_t *status,
                        hipStream_t s);
int launch_radius_attach(int64_t N, const float *sorted, const int32_t *cell_start, const float *lo, float h, const int32_t *dims,
                         const int32_t *group, float r2, const int32_t *count, int min_points, int32_t *attach, hipStream_t s);
int launch_components_flatten(int64_t N, const int32_t *count, int min_points, const int32_t *attach, int32_t *parent, int32_t *root,
                              int32_t *status, hipStream_t s);
// regions over a neighbour list by feature similarity (regions.hip): the cosine of every listed pair and each row's liveness, then
// the union-find of union_find.h over the edges that pass; launch_components_flatten reads the roots.  dist / group may be nullptr
int launch_neighbor_similarity(int64_t N, int D, int k, const int32_t *idx, const void *F, int mt, int64_t ldf, float *sim,
                               int32_t *live, hipStream_t s);
int launch_edge_union(int64_t N, int k, const int32_t *idx, const float *sim, const int32_t *live, const float *dist,
                      const int32_t *group, float sim_min, float max_dist, int32_t *count, int32_t *parent, int32_t *status,
                      hipStream_t s);
// a field asked at arbitrary 3-D points (sample.hip): the packed Gaussians in the grid's sorted order, each query's k Gaussians of
// largest weight, the field blended over such a list, and the weighted vote of a label field.  live / visited may be nullptr
int launch_gaussian_pack(int64_t N, const float *means, int64_t ldm, const float *quats, int64_t ldq, const float *scales, int64_t lds_,
                         const float *opac, const uint8_t *live, const int64_t *perm, float *pack, hipStream_t s);
int launch_point_gaussians(const float *sorted, const int32_t *cell_start, const float *lo, float h, const int32_t *dims,
                           const float *pack, float r2, float alpha_min, int64_t Q, const float *queries, int64_t ldq,
                           const int64_t *order, int k, int32_t *idx, float *w, int32_t *n_contrib, int32_t *visited, hipStream_t s);
int launch_neighbor_blend(int64_t Q, int64_t M, int D, int k, const int32_t *idx, const float *w, const void *F, int mt, int64_t ldf,
                          void *out, int ot, int64_t ldo, float *wsum, hipStream_t s);
int launch_weighted_vote(int64_t Q, int64_t M, int k, const int32_t *idx, const float *w, const int32_t *labels, int K,
                         int32_t *out_label, float *out_share, hipStream_t s);
// PCA of a finished field (pca.hip): column means, centred Gram, projection onto k <= 16 components, colours.  ws: the caller's
// pca_workspace_bytes(N, D) bytes (the slices' partial sums), free again when the call's kernels have run.
size_t pca_workspace_bytes(int64_t N, int D);
int launch_column_means(int64_t N, int D, const void *X, int mt, int64_t ldx, float *mean, void *ws, hipStream_t s);
int launch_centered_gram(int64_t N, int D, const void *X, int mt, int64_t ldx, const float *mean, double *gram, void *ws,
                         hipStream_t s);
int launch_pca_project(int64_t N, int D, int k, const void *X, int mt, int64_t ldx, const float *mean, const float *V, float *Y,
                       float *minmax, hipStream_t s);
int launch_pca_colors(int64_t n, const float *Y, const float *lo_hi, float *colors, hipStream_t s);
// clustering a finished field (cluster.hip): the k-means assignment (k_knn_search's score + a per-centroid bias, argmax only) and
// the per-cluster float64 column sums of rows grouped by the caller.  ws: the caller's cluster_workspace_bytes(N, D, K) bytes.
int launch_kmeans_assign(int64_t N, int K, int D, const void *X, int mt, int64_t ldx, const float *C, int64_t ldc, const float *bias,
                         int32_t *label, float *best, hipStream_t s);
size_t cluster_workspace_bytes(int64_t N, int D, int K);
int launch_cluster_sums(int64_t N, int D, int K, const void *X, int mt, int64_t ldx, const float *w, const int64_t *order,
                        const int64_t *start, double *sums, double *wsum, void *ws, hipStream_t s);
// questions asked of a finished field (query.hip): prompt scores + 3-D mask in one pass over X; the field rendered at M pixels
// of a projected and sorted view.  threshold: host pointer or nullptr.
int launch_prompt_scores(int64_t N, int D, int P, int n_pos, const void *X, int mt, int64_t ldx, const float *prompts, int normalize,
                         const float *threshold, uint8_t *mask, float *scores, hipStream_t s);
// the fp16 / bf16 instantiations of k_prompt_scores (query_half.hip); the caller checks the launch
void launch_prompt_scores_half(unsigned grid, hipStream_t s, int64_t N, int D, int P, int n_pos, const void *X, int mt, int64_t ldx,
                               const float *prompts, int normalize, int use_thr, float thr, uint8_t *mask, float *scores);
int launch_probe_pixels(const Ws &W, const ViewDev &V, int M, const int32_t *xy, const void *X, int mt, int64_t ldx, int D, float *out,
                        float *depth, float *alpha, hipStream_t s);
void launch_probe_pixels_half(const Ws &W, const ViewDev &V, int M, const int32_t *xy, const void *X, int mt, int64_t ldx, int D,
                              float *out, float *depth, float *alpha, hipStream_t s);
// the Gaussians a pixel is made of (pixels.hip): xy == nullptr: every pixel of the view, else the M pixels of xy; ids and weights
// [P, k], the four per-pixel outputs may be nullptr
int launch_pixel_gaussians(const Ws &W, const ViewDev &V, int k, int M, const int32_t *xy, int32_t *ids, float *weights,
                           int32_t *n_contrib, float *alphas, int32_t *median_id, float *median_depth, hipStream_t s);
int launch_dump_pairs(const Layout &L, const Ws &W, const ViewDev &V, int64_t cap, int32_t *gid, int32_t *pix,
                      float *w, u64 *n_dev, hipStream_t s);
int launch_accum_stats(const Ws &W, gwbp_stats *accum, hipStream_t s);

// ---- device helpers -----------------------------------------------------------------------------------------
#ifdef __HIPCC__
__device__ __forceinline__ float dot3f(float a0, float a1, float a2, float b0, float b1, float b2)
{
    return __builtin_fmaf(a2, b2, __builtin_fmaf(a1, b1, a0 * b0));
}

// exp(x), x <= 0: ln2 hi/lo range reduction, degree-7 Taylor (Horner, fma), exponent added to the bit pattern.
// Deterministic (no v_exp_f32), so weights do not depend on a transcendental unit; ~12 VALU ops.
__device__ __forceinline__ float exp_neg_core(float x) // -80 <= x <= 0
{
    const float t = x * 0x1.715476p+0f;
    const float n = __builtin_rintf(t);
    float r = __builtin_fmaf(n, -0x1.62e4p-1f, x);
    r = __builtin_fmaf(n, -0x1.7f7d1cp-20f, r);
    float p = 0x1.a01a02p-13f;
    p = __builtin_fmaf(p, r, 0x1.6c16c2p-10f);
    p = __builtin_fmaf(p, r, 0x1.111112p-7f);
    p = __builtin_fmaf(p, r, 0x1.555556p-5f);
    p = __builtin_fmaf(p, r, 0x1.555556p-3f);
    p = __builtin_fmaf(p, r, 0.5f);
    p = __builtin_fmaf(p, r, 1.0f);
    p = __builtin_fmaf(p, r, 1.0f);
    return __int_as_float(__float_as_int(p) + (((int)n) << 23));
}
__device__ __forceinline__ float exp_neg(float x)
{
    return exp_neg_core(__builtin_fmaxf(x, -80.0f));
}
// exp_neg(-fmaxf(sigma, 0)) bit for bit with ONE clamp instruction: med3(-sigma, 0, -80) is -sigma inside [0, 80], 0 below
// (exp of either zero is 1.0) and -80 above; fmaxf twice costs three (each with a canonicalising v_max in front).
__device__ __forceinline__ float exp_neg_sigma(float sigma)
{
    return exp_neg_core(__builtin_amdgcn_fmed3f(-sigma, 0.0f, -80.0f));
}

__device__ __forceinline__ int lane_id() { return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
__device__ __forceinline__ u32 mbcnt(u64 mask)
{
    return __builtin_amdgcn_mbcnt_hi((u32)(mask >> 32), __builtin_amdgcn_mbcnt_lo((u32)mask, 0u));
}
// GWBP_FLAG_FRONT_PRIORITY: the front-stage kernels (project / sort / blend of view v+1) raise their waves' issue
// priority.  Beside the persistent scatter kernel of view v the SIMD arbiter otherwise serves the four older scatter waves
// first and the front's dependent instruction chains stretch 3x (k_blend 1.0 -> 2.9 ms at equal occupancy).
#ifndef GWBP_FRONT_PRIO
#define GWBP_FRONT_PRIO 3 // (levels 1, 2 and 3 measured equal at C2, round 5: 3.43-3.45 ms/view each; 0 = off costs 4 %)
#endif
__device__ __forceinline__ void front_priority(int on)
{
    if (on)
        __builtin_amdgcn_s_setprio(GWBP_FRONT_PRIO);
}
// Sum over the 64 lanes, returned wave-uniform: four DPP adds inside each row of 16 lanes, then the four row totals.
template <int CTRL>
__device__ __forceinline__ float dpp_f(float x)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float wave_sum(float v)
{
    v += dpp_f<0xB1>(v);  // quad_perm [1,0,3,2]
    v += dpp_f<0x4E>(v);  // quad_perm [2,3,0,1]
    v += dpp_f<0x141>(v); // row_half_mirror
    v += dpp_f<0x140>(v); // row_mirror
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return (r0 + r1) + (r2 + r3);
}
// wave_sum for a double: the two halves move through the same DPP controls.
template <int CTRL>
__device__ __forceinline__ double dpp_d(double x)
{
    const long long b = __double_as_longlong(x);
    const u32 lo = (u32)__builtin_amdgcn_update_dpp(0, (int)(u32)b, CTRL, 0xF, 0xF, true);
    const u32 hi = (u32)__builtin_amdgcn_update_dpp(0, (int)(u32)(b >> 32), CTRL, 0xF, 0xF, true);
    return __longlong_as_double((long long)(((u64)hi << 32) | lo));
}
__device__ __forceinline__ double lane_d(double x, int l)
{
    const long long b = __double_as_longlong(x);
    const u32 lo = (u32)__builtin_amdgcn_readlane((int)(u32)b, l), hi = (u32)__builtin_amdgcn_readlane((int)(u32)(b >> 32), l);
    return __longlong_as_double((long long)(((u64)hi << 32) | lo));
}
__device__ __forceinline__ double wave_sum_d(double v)
{
    v += dpp_d<0xB1>(v);  // quad_perm [1,0,3,2]
    v += dpp_d<0x4E>(v);  // quad_perm [2,3,0,1]
    v += dpp_d<0x141>(v); // row_half_mirror
    v += dpp_d<0x140>(v); // row_mirror
    return (lane_d(v, 0) + lane_d(v, 16)) + (lane_d(v, 32) + lane_d(v, 48));
}
// ---- feature-map element types (GWBP_MAP_*) ------------------------------------------------------------------------------
// A half map is widened to fp32 exactly where the staging writes it into LDS (or, for a value used at once, where it is
// loaded): slabs, sums and F / d stay fp32.  `raw` is what a load lands; `land` keeps a loaded scalar's bits in a 32-bit
// register (the 256-channel kernel's landing area is float-typed) and `widen` turns those bits into the value; `cvt4` widens
// the four channels of one `raw4` (float4, or the four 16-bit halves of a uint2).  For GWBP_MAP_F32 all of it is the identity.
template <int MT>
struct MapElem;
template <>
struct MapElem<GWBP_MAP_F32> {
    typedef float raw;
    typedef float4 raw4;
    static __device__ __forceinline__ float cvt(float x) { return x; }
    static __device__ __forceinline__ float land(float x) { return x; }
    static __device__ __forceinline__ float widen(float x) { return x; }
    static __device__ __forceinline__ float4 cvt4(float4 x) { return x; }
};
template <>
struct MapElem<GWBP_MAP_F16> {
    typedef unsigned short raw;
    typedef uint2 raw4;
    static __device__ __forceinline__ float cvt(unsigned short x) { return (float)__builtin_bit_cast(_Float16, x); }
    static __device__ __forceinline__ float land(unsigned short x) { return __uint_as_float((u32)x); }
    static __device__ __forceinline__ float widen(float b) { return cvt((unsigned short)__float_as_uint(b)); }
    static __device__ __forceinline__ float4 cvt4(uint2 x)
    {
        return make_float4(cvt((unsigned short)x.x), cvt((unsigned short)(x.x >> 16)), cvt((unsigned short)x.y),
                           cvt((unsigned short)(x.y >> 16)));
    }
};
template <>
struct MapElem<GWBP_MAP_BF16> {
    typedef unsigned short raw;
    typedef uint2 raw4;
    static __device__ __forceinline__ float cvt(unsigned short x) { return __uint_as_float((u32)x << 16); }
    static __device__ __forceinline__ float land(unsigned short x) { return __uint_as_float((u32)x); }
    static __device__ __forceinline__ float widen(float b) { return __uint_as_float(__float_as_uint(b) << 16); }
    static __device__ __forceinline__ float4 cvt4(uint2 x)
    {
        return make_float4(__uint_as_float(x.x << 16), __uint_as_float(x.x & 0xFFFF0000u), __uint_as_float(x.y << 16),
                           __uint_as_float(x.y & 0xFFFF0000u));
    }
};

// Four consecutive floats of row `p` (nullptr: a row beyond the matrix) at column c, zero beyond D.  VEC: rows are 16-B aligned.
template <bool VEC>
__device__ __forceinline__ float4 load4(const float *__restrict__ p, int c, int D)
{
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!p)
        return v;
    if (VEC && c + 4 <= D)
        return *reinterpret_cast<const float4 *>(p + c);
    if (c < D)
        v.x = p[c];
    if (c + 1 < D)
        v.y = p[c + 1];
    if (c + 2 < D)
        v.z = p[c + 2];
    if (c + 3 < D)
        v.w = p[c + 3];
    return v;
}
// ... and written: the columns of v that lie below D.
template <bool VEC>
__device__ __forceinline__ void store4(float *__restrict__ p, int c, int D, float4 v)
{
    if (VEC && c + 4 <= D) {
        *reinterpret_cast<float4 *>(p + c) = v;
        return;
    }
    if (c < D)
        p[c] = v.x;
    if (c + 1 < D)
        p[c + 1] = v.y;
    if (c + 2 < D)
        p[c + 2] = v.z;
    if (c + 3 < D)
        p[c + 3] = v.w;
}

// The same four columns of a row of a finished FIELD whose elements have type MT (GWBP_MAP_*), zero beyond D, no load for a null
// row, in two steps so that a kernel can keep loads in flight: load4raw lands the BITS (MapElem<MT>::raw4: a float4, or the four
// packed halves in a uint2; zero bits are +0 in every type) and widen4 turns them into four fp32 values (exact) where they are
// used -- a conversion next to the load would make the wave wait for the load there.  VEC, half rows: ONE 8-B load -- the row address
// is 8-B aligned, the row stride a multiple of 4 elements and c a multiple of 4; otherwise 2-B element loads, packed.  For
// GWBP_MAP_F32 load4raw IS load4 and widen4 the identity: a kernel's fp32 instantiation compiles to what it was before it had a
// typed operand.  load4t is both at once, for a value used where it is loaded.
template <int MT, bool VEC>
__device__ __forceinline__ typename MapElem<MT>::raw4 load4raw(const void *__restrict__ row, int c, int D)
{
    if constexpr (MT == GWBP_MAP_F32) {
        return load4<VEC>(static_cast<const float *>(row), c, D);
    } else {
        const unsigned short *p = static_cast<const unsigned short *>(row);
        if (!p)
            return make_uint2(0u, 0u);
        if (VEC && c + 4 <= D)
            return *reinterpret_cast<const uint2 *>(p + c);
        u32 e0 = 0u, e1 = 0u, e2 = 0u, e3 = 0u;
        if (c < D)
            e0 = p[c];
        if (c + 1 < D)
            e1 = p[c + 1];
        if (c + 2 < D)
            e2 = p[c + 2];
        if (c + 3 < D)
            e3 = p[c + 3];
        return make_uint2(e0 | (e1 << 16), e2 | (e3 << 16));
    }
}
template <int MT>
__device__ __forceinline__ float4 widen4(typename MapElem<MT>::raw4 r)
{
    return MapElem<MT>::cvt4(r);
}
template <int MT, bool VEC>
__device__ __forceinline__ float4 load4t(const void *__restrict__ row, int c, int D)
{
    return widen4<MT>(load4raw<MT, VEC>(row, c, D));
}

// The host side of a typed operand: a launcher turns its run-time element type mt (GWBP_MAP_*, checked by the C ABI layer) and "the
// rows take the vector path" into template arguments HERE, so that each kernel's launch line is written once:
//     with_field_type(mt, vec, [&](auto MT, auto VEC) { hipLaunchKernelGGL((k<MT, VEC>), ..., field_ptr<MT>(X), ...); });
template <class Fn>
auto with_map_type(int mt, Fn &&fn)
{
    if (mt == GWBP_MAP_F16)
        return fn(std::integral_constant<int, GWBP_MAP_F16>{});
    if (mt == GWBP_MAP_BF16)
        return fn(std::integral_constant<int, GWBP_MAP_BF16>{});
    return fn(std::integral_constant<int, GWBP_MAP_F32>{});
}
template <class Fn>
auto with_bool(bool b, Fn &&fn)
{
    if (b)
        return fn(std::true_type{});
    return fn(std::false_type{});
}
template <class Fn>
auto with_field_type(int mt, bool vec, Fn &&fn)
{
    return with_map_type(mt, [&](auto MT) { return with_bool(vec, [&](auto VEC) { return fn(MT, VEC); }); });
}
template <int MT>
const typename MapElem<MT>::raw *field_ptr(const void *p)
{
    return static_cast<const typename MapElem<MT>::raw *>(p);
}

// One fp32 value rounded ONCE, to nearest even, to the element type OT of a typed output (k_finalize): torch's x.to(dtype) bit for
// bit.  bf16 in integer arithmetic on the fp32 bits (a NaN becomes the quiet NaN 0x7FC0, an infinity stays one, a carry out of the
// mantissa is the correct rounding up to the next binade or to infinity); fp16 is the compiler's conversion, subnormal results kept.
template <int OT>
__device__ __forceinline__ typename MapElem<OT>::raw narrow(float x)
{
    if constexpr (OT == GWBP_MAP_F32) {
        return x;
    } else if constexpr (OT == GWBP_MAP_F16) {
        return __builtin_bit_cast(unsigned short, (_Float16)x);
    } else {
        const u32 b = __float_as_uint(x);
        if ((b & 0x7FFFFFFFu) > 0x7F800000u)
            return (unsigned short)0x7FC0u;
        return (unsigned short)((b + 0x7FFFu + ((b >> 16) & 1u)) >> 16);
    }
}

// store4 for a row of a typed OUTPUT: the columns of v below D, each narrow<OT>'d.  VEC, half rows: ONE 8-B store (load4raw's rule: the
// row address 8-B aligned, the row stride a multiple of 4 elements, c a multiple of 4).  For GWBP_MAP_F32 it IS store4.
template <int OT, bool VEC>
__device__ __forceinline__ void store4t(void *__restrict__ row, int c, int D, float4 v)
{
    if constexpr (OT == GWBP_MAP_F32) {
        store4<VEC>(static_cast<float *>(row), c, D, v);
    } else {
        unsigned short *p = static_cast<unsigned short *>(row);
        const unsigned short e0 = narrow<OT>(v.x), e1 = narrow<OT>(v.y), e2 = narrow<OT>(v.z), e3 = narrow<OT>(v.w);
        if (VEC && c + 4 <= D) {
            *reinterpret_cast<uint2 *>(p + c) = make_uint2((u32)e0 | ((u32)e1 << 16), (u32)e2 | ((u32)e3 << 16));
            return;
        }
        if (c < D)
            p[c] = e0;
        if (c + 1 < D)
            p[c + 1] = e1;
        if (c + 2 < D)
            p[c + 2] = e2;
        if (c + 3 < D)
            p[c + 3] = e3;
    }
}
template <int OT>
typename MapElem<OT>::raw *out_ptr(void *p)
{
    return static_cast<typename MapElem<OT>::raw *>(p);
}

__device__ __forceinline__ u32 uniform(u32 v) { return (u32)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ u64 uniform64(u64 v)
{
    return ((u64)uniform((u32)(v >> 32)) << 32) | uniform((u32)v);
}
#endif

} // namespace gwbp
