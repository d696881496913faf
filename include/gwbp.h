/*
 * gwbp.h -- C ABI of libgwbp.so: gradient-weighted feature back-projection on MI355X (gfx950).
 *
 * This is the drop-in boundary for the one hot path this repository implements.  In the reference
 * (JojiJoseph/3dgs-gradient-backprojection) the boundary is the Python operator
 *     gsplat.rasterization(means, quats, scales, opacities, colors, viewmats, Ks, width, height, ...)
 * called at backproject.py:89,115,133 (and :223,251,271; backproject_compressed.py:102,129,147;
 * utils.py:238,316,329) followed by autograd backward (backproject.py:129,147).  gsplat's own native
 * boundary is a pybind11/torch extension taking at::Tensor; the replacement is a plain C ABI:
 * raw device pointers, sizes, a hipStream_t passed as void*, int status codes, no C++ types, no torch types.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _host; fp32 arrays are dense row-major
 *   - the caller owns every buffer, including the workspace; the library allocates nothing persistent and
 *     keeps no global mutable state except a thread-local last-error string and two per-device-ordinal caches of
 *     device facts (CU count; "dynamic-LDS limit raised for kernel k") -- work is launched on the CURRENT HIP device,
 *     which must be the device of `stream` and of every pointer
 *   - no environment variable is read (ablation knobs exist only in a -DGWBP_PROFILE build, `make PROFILE=1`)
 *   - every entry point only ENQUEUES work on `stream` (no host synchronisation) unless documented
 *   - return value: 0 = ok, <0 = GWBP_E* (invalid argument / workspace too small), >0 = hipError_t
 *   - quats are (w,x,y,z) and need not be normalised; scales/opacities are post-activation
 *     (backproject.py:55-57); viewmat is row-major 4x4 world->camera [R|t] (utils.py:215-219);
 *     K is row-major 3x3
 *
 * Thread-safety: re-entrant; one host thread per GPU process is the expected caller.
 */
#ifndef GWBP_H
#define GWBP_H

#include <stddef.h>
#include <stdint.h>

/* The library is built with -fvisibility=hidden: the entry points below are its ONLY dynamic symbols (no C++ symbol of the
 * implementation -- launchers taking hipStream_t, kernel host stubs -- crosses the boundary; tests/test_capi_cpu.py compares
 * `nm -D --defined-only` with this header, both directions). */
#if defined(__GNUC__) || defined(__clang__)
#define GWBP_API __attribute__((visibility("default")))
#else
#define GWBP_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define GWBP_OK 0
#define GWBP_EINVAL (-1)    /* bad argument (null pointer, non-positive size, unsupported tile size, ...) */
#define GWBP_EWORKSPACE (-2) /* workspace smaller than gwbp_workspace_size() reports */
#define GWBP_EUNSUPPORTED (-3)

#define GWBP_TILE 16 /* gsplat tile_size default; the tile rectangle rule is part of the numerics */

/* Per-view parameters (host struct, passed by pointer, copied at call time). Mirrors the keyword defaults of
 * gsplat.rasterization(): near_plane=0.01, far_plane=1e10, radius_clip=0.0, eps2d=0.3, tile_size=16. */
typedef struct gwbp_view {
    float viewmat[16]; /* row-major world->camera */
    float K[9];        /* row-major intrinsics */
    int32_t width, height;
    float near_plane, far_plane, eps2d, radius_clip;
} gwbp_view;

/* Capacities the caller chooses for the variable-size intermediates of one view. */
typedef struct gwbp_caps {
    int64_t n_gaussians; /* N */
    int64_t isect_cap;   /* max (Gaussian, tile) intersections per view */
    int64_t pair_cap;    /* max stored weight-store entries (8 B each) per view, incl. page slack */
    int32_t max_width, max_height;
    /* Tuning: number of persistent scatter workgroups (rounded up to a multiple of 8); 0 = one per CU (default and
     * measured optimum on MI355X, also when the next view's front stages overlap on a second stream). */
    int32_t scatter_workgroups;
    /* GWBP_FLAG_* bits; 0 = gsplat's exact tile binning (3-sigma square, what meta["isect_ids"] must show). */
    int32_t flags;
} gwbp_caps;

/* Bin every Gaussian only into the tiles that the bounding box of its alpha >= 1/255 ellipse touches (clipped to the
 * 3-sigma square): low-opacity and elongated Gaussians enter fewer tile lists.  A dropped (Gaussian, tile) pair has no
 * pixel with alpha >= 1/255 (5 % + 1 px margin), so F, d, the weight store and every render are unchanged bit for bit;
 * only n_isect and the sorted intersection lists shrink.  Used by the fused back-projection path. */
#define GWBP_FLAG_TIGHT_BINNING 1
/* The kernels of gwbp_project / gwbp_bin_sort / gwbp_blend_weights run at raised wave priority.  For callers that run
 * them on a second stream beside gwbp_scatter of the previous view when D % 256 == 0 (the 256-channel scatter kernel
 * leaves issue slots the front can only use with priority; with the 128-channel kernel the flag costs time). */
#define GWBP_FLAG_FRONT_PRIORITY 2
/* gwbp_scatter uses the 128-channel kernel even when D % 256 == 0.  The 256-channel kernel needs fewer vector
 * instructions per (pair, channel) but more work per (Gaussian, tile) record: it wins when records are long (C2: 48
 * pairs per record, -5 % per view) and loses when they are short and the flush atomics dominate (C4: 25 pairs per
 * record, +5 %).  The host decides from the first view's gwbp_stats (n_pairs / n_headers).  gwbp_blend_weights skips
 * the half-tile record lists (15-20 % of its time) when the flag is set, so a view blended WITH the flag must be
 * scattered with it; the other direction (blend without, scatter with) is fine. */
#define GWBP_FLAG_NARROW_SCATTER 4
/* gwbp_blend_scatter_encoded runs its producer / consumer form: ONE persistent workgroup per CU whose two encoder waves stream
 * tile after tile through the matrix cores into a ring of encoded tiles in LDS while its fourteen blend waves drain
 * it -- the HBM-bound encoder stream and the issue-bound blend loops run concurrently for the whole launch instead of one after
 * the other in every wave.  Same encoded pixels and weights bit for bit; F and d differ by summation order only.  Pays on images of
 * many tiles per CU (C5: 6700 tiles on 256 CUs). */
#define GWBP_FLAG_SPLIT_ENCODER 16
/* (bit 3 was GWBP_FLAG_GROUP_SCATTER, an experimental block-sparse scatter on the matrix cores: measured slower than the
 * vector kernels and removed; unknown flag bits are rejected with GWBP_EINVAL.) */

/* Device-resident per-view counters, readable after the stream has drained (gwbp_read_stats).  gwbp_project (or
 * gwbp_project_camera) zeroes them.  n_pairs, n_headers, pool_used and reserved describe the view's LAST blend: a blend repeated
 * on one projection reports what it alone counted, and starts from an empty weight pool.  The overflow bits are sticky: once set,
 * they stay set until the next gwbp_project of a view on this workspace. */
typedef struct gwbp_stats {
    uint64_t n_pairs;     /* contributing (Gaussian, pixel) pairs = sum over pixels of #weights */
    uint32_t n_isect;     /* (Gaussian, tile) intersections emitted */
    uint32_t n_visible;   /* Gaussians surviving projection culling */
    uint32_t n_headers;   /* (Gaussian, tile) pairs with at least one contributing pixel */
    uint32_t pool_used;   /* weight-pool entries a uniform shard capacity would need: kShards x fullest shard */
    uint32_t overflow;    /* bit0: isect_cap exceeded, bit1: pair_cap exceeded -> results of this view invalid;
                           * (bit0: n_isect reads 0 and every later stage sees an EMPTY view.  bit1: the blend itself completes --
                           * its alpha map is right and n_pairs keeps counting past the exhausted pool, so it is the count an ample
                           * pool would report and a caller can size its retry from it; the store, n_headers and pool_used of that
                           * blend are undefined)
                           * bit4: internal error -- a wave of gwbp_blend_scatter_encoded's producer / consumer form gave up waiting on
                           * its ring of encoded tiles (the launch ends instead of hanging; the view's result is invalid);
                           * bit3: gwbp_blend_tokens met a tile that spans more than 2 x 2 tokens (precondition violated) -> invalid;
                           * bit2: gwbp_scatter / gwbp_accumulate_d asked for the 256-channel kernel on a view that was
                           * blended WITH GWBP_FLAG_NARROW_SCATTER (no half-tile lists / weight sums): that call left
                           * F and d untouched -- scatter again with the flag set; also set by gwbp_scatter_labels (and
                           * gwbp_scatter_tokens) on a workspace that holds no weight store (token sums): F and d untouched */
    uint32_t reserved;    /* what the last blend of this view left: 0 = weight store, 1 = store + half-tile lists, 2 = nothing (gwbp_blend_scatter), 3 = token-quadrant weight sums (gwbp_blend_tokens) */
} gwbp_stats;

/* Library / build identification ("gfx950;<git-less build tag>"). */
GWBP_API const char *gwbp_version(void);
/* Thread-local description of the last non-zero status returned on this thread. */
GWBP_API const char *gwbp_last_error_string(void);

/* Bytes of workspace needed for the given capacities (256-B aligned sub-buffers). */
GWBP_API int gwbp_workspace_size(const gwbp_caps *caps, size_t *bytes_host);

/* ---- stage entry points (replace the stages inside gsplat.rasterization) -------------------- */

/* fully_fused_projection + tiles-per-Gaussian count.  Writes the projected table inside the workspace and,
 * if non-null, user-visible copies: radii[N] int32 (0 = culled), means2d[N,2], depths[N], conics[N,3]. */
GWBP_API int gwbp_project(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                 const float *means, const float *quats, const float *scales, const float *opacities,
                 int32_t *radii, float *means2d, float *depths, float *conics, void *stream);

/* Camera models and rasterize modes of gwbp_project_camera (gsplat.rasterization's camera_model / rasterize_mode). */
#define GWBP_CAMERA_PINHOLE 0 /* u = fx x / z + cx; x/z, y/z clamped to the frustum + 30 % margin inside the Jacobian */
#define GWBP_CAMERA_ORTHO 1   /* u = fx x + cx, v = fy y + cy; J = [[fx, 0, 0], [0, fy, 0]] */
#define GWBP_CAMERA_FISHEYE 2 /* ideal equidistant: u = fx x theta / rho + cx, rho = |(x, y)|, theta = atan2(rho, z); no
                               * distortion coefficients; exact Jacobian of that map */
#define GWBP_RASTERIZE_CLASSIC 0
#define GWBP_RASTERIZE_ANTIALIASED 1 /* opacity x compensation, compensation = sqrt(det(S) / det(S + eps2d I)) of the 2-D
                                      * covariance S; radius, culling and conic as in classic */

/* gwbp_project under a camera model and a rasterize mode.  Everything downstream (bin_sort, every blend / scatter / render
 * entry point) reads the projected table it writes, so it takes the place of gwbp_project for the view; under
 * GWBP_RASTERIZE_ANTIALIASED the table holds the compensated opacities (as does the GWBP_FLAG_TIGHT_BINNING bound).
 * compensations[N] (optional) is gsplat's meta["compensations"]: written under GWBP_RASTERIZE_ANTIALIASED only, 0 for culled
 * Gaussians.
 * Equal to gwbp_project bit for bit for (GWBP_CAMERA_PINHOLE, GWBP_RASTERIZE_CLASSIC).  An unknown model or mode is
 * GWBP_EINVAL, checked before anything else.  gwbp_backproject_view stays pinhole / classic. */
GWBP_API int gwbp_project_camera(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                 int32_t camera_model, int32_t rasterize_mode, const float *means, const float *quats, const float *scales,
                 const float *opacities, int32_t *radii, float *means2d, float *depths, float *conics,
                 float *compensations, void *stream);

/* isect_tiles + stable radix sort by (tile, depth) + isect_offset_encode.  Optional outputs:
 * isect_ids[isect_cap] int64 sorted keys, flatten_ids[isect_cap] int32, tile_offsets[tiles+1] int32. */
GWBP_API int gwbp_bin_sort(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                  int64_t *isect_ids, int32_t *flatten_ids, int32_t *tile_offsets, void *stream);

/* rasterize_to_pixels forward, weights only: per tile, front-to-back blend producing the sparse weight store
 * (w = alpha*T per contributing (Gaussian, pixel)) inside the workspace; alphas[H*W] (= 1 - T) optional. */
GWBP_API int gwbp_blend_weights(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                       float *alphas, void *stream);

/* gwbp_blend_weights that also adds the view's denominators, d[g] += scale_d * sum_p w_g(p), while it writes each
 * record (needs caps WITHOUT GWBP_FLAG_NARROW_SCATTER): what a caller that overlaps the front stage of view v+1 with
 * the scatter of view v uses on the front's stream (then d = NULL for gwbp_scatter) -- the whole denominator pass of
 * backproject.py:133-150 costs one 4-B atomic per (Gaussian, tile) record and no kernel of its own. */
GWBP_API int gwbp_blend_weights_d(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                         float *alphas, float scale_d, float *d, void *stream);

/* Blend AND scatter of one view in one kernel, for narrow maps (1 <= D <= 16; on images of at most 4096 tiles, where a wave
 * takes a quarter tile with one pixel per lane, 1 <= D <= 32: backproject_compressed.py:127-165 after its
 * 512 -> 16 encoder; a 3-channel colour gradient): while a tile is blended its 256 pixels x D channels sit in registers,
 * each contributing (Gaussian, tile) record's sums  F[g, :D] += scale_f * sum_p w f[p, :],  d[g] += scale_d * sum_p w  are
 * reduced across the wave and added with one atomic instruction.  No weight store is written (the workspace's store is
 * left EMPTY: a later gwbp_scatter / gwbp_render of this view adds nothing and gwbp_stats.reserved reads 2), no scatter
 * kernel runs.  feats[y * fs_y + x * fs_x + c] full resolution, unit channel stride; d may be NULL; alphas optional.
 * The weights are those of gwbp_blend_weights bit for bit; F and d differ from gwbp_scatter's only by summation order. */
GWBP_API int gwbp_blend_scatter(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                       const float *feats, int64_t fs_y, int64_t fs_x, int32_t D, float scale_f, float scale_d,
                       float *F, float *d, float *alphas, void *stream);

/* gwbp_blend_scatter of feats[H, W, K] @ encoder[K, n_out] (backproject_compressed.py:127-165 in ONE kernel): every tile's wave
 * first streams its 256 pixels x K channels once through the matrix cores (exact fp32, the k-ordered chain of gwbp_encode_map)
 * and keeps the n_out <= 16 outputs per pixel in registers -- no [H, W, n_out] map, no encoder kernel -- then blends and
 * scatters like gwbp_blend_scatter.  feats[y * fs_y + x * fs_x + k]: channel-contiguous 16-B aligned pixels, K % 16 == 0,
 * 16 <= K <= 512; encoder row-major [K, n_out].  Any image size.  Results equal gwbp_encode_map + gwbp_blend_scatter bit for
 * bit in the encoded pixels, hence in every weight and (up to summation order) in F and d. */
GWBP_API int gwbp_blend_scatter_encoded(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                               const float *feats, int64_t fs_y, int64_t fs_x, int32_t K, const float *encoder, int32_t n_out,
                               float scale_f, float scale_d, float *F, float *d, float *alphas, void *stream);

/* The dino variant in TOKEN space (backproject.py:242-289: 64 x 64 x 1024 patch tokens, F.interpolate(mode="nearest") to the
 * view's size, then the back-projection).  All pixels of a token carry the same vector, so F_v[g,:] = sum_t omega_{g,t} tok[t,:]
 * with omega_{g,t} = sum_{p in t} w_g(p).  gwbp_blend_tokens is gwbp_blend_weights whose product is those sums instead of a
 * weight store: per contributing (Gaussian, tile) record the weight sums of the tile's (at most) 2 x 2 tokens, filed at the
 * record's emit position so that the sums of one Gaussian lie back to back.  gwbp_scatter_tokens then adds
 *     F[g,:] += scale_f * sum_t omega_{g,t} tokens[t,:],   d[g] += scale_d * sum_t omega_{g,t}
 * with ONE plain read-modify-write of every row that receives weight: no atomics, no weight store, deterministic.
 * PRECONDITION: ymap[view.height] / xmap[view.width] (int32 device arrays, PyTorch's nearest rule, non-decreasing) send the 16
 * pixels of any tile row / column to at most TWO consecutive tokens, i.e. a token is at least a tile wide and high
 * (16 * lr_w <= width and 16 * lr_h <= height suffice); a tile that violates it sets gwbp_stats.overflow bit 3 and the view's
 * result is invalid -- use gwbp_scatter_upsampled for finer maps.  The weights are gwbp_blend_weights' bit for bit (the alpha map
 * too); F and d equal gwbp_scatter_upsampled's up to summation order.  After gwbp_blend_tokens the workspace holds NO weight
 * store (gwbp_stats.reserved reads 3): gwbp_scatter / gwbp_render of that view add nothing.
 * gwbp_scatter_tokens: tokens[row * ts_y + col * ts_x + c], channel-contiguous 16-B aligned rows, D % 4 == 0 (256-channel chunks,
 * the last one masked; GWBP_EUNSUPPORTED otherwise), views of at most 4096 x 4096 pixels; d may be NULL;
 * needs gwbp_project + gwbp_bin_sort + gwbp_blend_tokens of the same view in this workspace (anything else sets overflow bit 2
 * and leaves F and d untouched). */
GWBP_API int gwbp_blend_tokens(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                               const int32_t *ymap, const int32_t *xmap, float *alphas, void *stream);
GWBP_API int gwbp_scatter_tokens(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                                 const float *tokens, int64_t ts_y, int64_t ts_x, int32_t D, const int32_t *ymap,
                                 const int32_t *xmap, float scale_f, float scale_d, float *F, float *d, void *stream);

/* ---- per-pixel weight maps (masks, confidences) ----------------------------------------------------------------
 * The _ex forms of the five blends take a map c(p) >= 0 at the view's resolution and weight what the view adds by it:
 *     F[g] += scale_f * sum_p w_g(p) c(p) f(p),     d[g] += scale_d * sum_p w_g(p) c(p)
 * -- the reference's per-view loop (backproject.py:115-151) with both of its targets multiplied by c.  The blend computes alpha
 * and T exactly as without a map (the alpha map is unchanged); what it adds or stores is w c(p), for pixels with c(p) != 0 only:
 * a pixel of weight 0 has no entry in the weight store, and a (Gaussian, tile) record left without one has no header.  Every
 * consumer of the blend (gwbp_scatter and its upsampled / bilinear / typed / encoded forms, gwbp_scatter_labels,
 * gwbp_accumulate_d, gwbp_scatter_tokens) is thereby weighted with no argument of its own.
 * Element (x, y) of the map is data[y * ws_y + x * ws_x] (strides in ELEMENTS, >= 0: a channel of an [H, W, C] tensor works).
 * GWBP_PIXW_U8 reads any non-zero byte as 1 (0 / 255 masks, bool tensors); the other types are values (negative or non-finite
 * values are carried through linearly / undefined).  reserved must be 0.  pixel_weights == NULL is the unweighted function, bit
 * for bit; the unweighted functions are these with NULL.  An unknown dtype, a NULL data, a negative stride or a non-zero reserved
 * returns GWBP_EINVAL before anything else is looked at. */
#define GWBP_PIXW_F32 0  /* float32 */
#define GWBP_PIXW_F16 1  /* IEEE binary16 */
#define GWBP_PIXW_BF16 2 /* bfloat16 */
#define GWBP_PIXW_U8 3   /* uint8 / bool: 0 or 1 */
typedef struct gwbp_pixel_weights {
    const void *data; /* device */
    int64_t ws_y, ws_x;
    int32_t dtype;    /* GWBP_PIXW_* */
    int32_t reserved; /* 0 */
} gwbp_pixel_weights;  /* 32 B */
GWBP_API int gwbp_blend_weights_ex(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                                   float *alphas, const gwbp_pixel_weights *pixel_weights, void *stream);
GWBP_API int gwbp_blend_weights_d_ex(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                                     float *alphas, float scale_d, float *d, const gwbp_pixel_weights *pixel_weights, void *stream);
GWBP_API int gwbp_blend_tokens_ex(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                                  const int32_t *ymap, const int32_t *xmap, float *alphas, const gwbp_pixel_weights *pixel_weights,
                                  void *stream);
GWBP_API int gwbp_blend_scatter_ex(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                                   const float *feats, int64_t fs_y, int64_t fs_x, int32_t D, float scale_f, float scale_d,
                                   float *F, float *d, float *alphas, const gwbp_pixel_weights *pixel_weights, void *stream);
GWBP_API int gwbp_blend_scatter_encoded_ex(const gwbp_caps *caps, void *workspace, size_t workspace_bytes,
                                           const gwbp_view *view_host, const float *feats, int64_t fs_y, int64_t fs_x, int32_t K,
                                           const float *encoder, int32_t n_out, float scale_f, float scale_d, float *F, float *d,
                                           float *alphas, const gwbp_pixel_weights *pixel_weights, void *stream);

/* ---- the view's RGB render as a by-product of the storing and token blends ---------------------------------------
 * The _rgb forms are the _ex functions above plus an RGB composite written while each tile is blended:
 *     image[p] = sum_g w_g(p) * colors[g]      (w = alpha * T, UNWEIGHTED even when pixel_weights is given)
 * accumulated front to back with fmaf(w, c, acc) exactly as gwbp_render_pixels does, so image equals gwbp_render_pixels(colors,
 * D = 3) of the same view bit for bit; no background.  colors is [N, 3] float32, image [H, W, 3] float32 (device, contiguous).
 * Everything else the blend produces (weight store, headers, d, token-quadrant sums, alphas) is unchanged bit for bit.
 * colors == NULL and image == NULL is the _ex function; exactly one of them NULL returns GWBP_EINVAL before anything else is
 * looked at (after the pixel weights).  The fused blends (gwbp_blend_scatter*) have no _rgb form: their blend needs the feature
 * map, which the network computes from this very render -- render those views with gwbp_render_pixels after gwbp_bin_sort. */
GWBP_API int gwbp_blend_weights_rgb(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                                    float *alphas, const gwbp_pixel_weights *pixel_weights, const float *colors, float *image,
                                    void *stream);
GWBP_API int gwbp_blend_weights_d_rgb(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                                      float *alphas, float scale_d, float *d, const gwbp_pixel_weights *pixel_weights,
                                      const float *colors, float *image, void *stream);
GWBP_API int gwbp_blend_tokens_rgb(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                                   const int32_t *ymap, const int32_t *xmap, float *alphas, const gwbp_pixel_weights *pixel_weights,
                                   const float *colors, float *image, void *stream);

/* d[g] += scale_d * sum_p w_g(p) alone, from the per-record weight sums gwbp_blend_weights left in the workspace
 * (needs a blend WITHOUT GWBP_FLAG_NARROW_SCATTER).  A caller that overlaps the front stage of view v+1 with the
 * scatter of view v issues it behind the blend on the front's stream and passes d = NULL to gwbp_scatter: the
 * denominators then cost nothing on the scatter's stream (backproject.py:133-150). */
GWBP_API int gwbp_accumulate_d(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                      float scale_d, float *d, void *stream);

/* What the reference obtains through backward(): F[g,:] += scale_f * sum_p w_g(p) * feats[p,:] and
 * d[g] += scale_d * sum_p w_g(p)   (backproject.py:127-131,145-150; scale = 1 for .sum(), 1/(H*W*D) and
 * 1/(H*W*3) for the dino .mean() variant, backproject.py:263,283).  feats is addressed as
 * feats[y*fs_y + x*fs_x + c*fs_c] (strides in floats; D % 128 == 0 or D <= 64 take the fast kernel; fs_c == 1 stages with 16-B loads).  d may be null. */
GWBP_API int gwbp_scatter(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                 const float *feats, int64_t fs_y, int64_t fs_x, int64_t fs_c, int32_t D, float scale_f,
                 float scale_d, float *F, float *d, void *stream);

/* The compressed variant in one kernel (backproject_compressed.py:127-165): gwbp_scatter of feats[H,W,K] @ encoder[K,D]
 * (D <= 16, K % 16 == 0, K <= 1024, channel-contiguous 16-B aligned pixels: feats[y*fs_y + x*fs_x + k]) without ever
 * writing the [H,W,D] map: every tile's pixels are read once, full width, and multiplied by the encoder (resident in LDS)
 * on the matrix cores while the tile's slab is staged (exact fp32: v_mfma_f32_16x16x4_f32). */
GWBP_API int gwbp_scatter_encoded(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                         const float *feats, int64_t fs_y, int64_t fs_x, int32_t K, const float *encoder, int32_t D,
                         float scale_f, float scale_d, float *F, float *d, void *stream);

/* gwbp_scatter over a LOW-RESOLUTION feature map that the reference would first upsample with
 * F.interpolate(mode="nearest") (dino variant, backproject.py:244-248): pixel (y, x) of the view reads
 * feats[ymap[y]*fs_y + xmap[x]*fs_x + c*fs_c].  ymap[view.height], xmap[view.width]: int32 device arrays (the host
 * side builds them with PyTorch's nearest rule: min(floor(i * in/out), in-1) in fp32).  Same result as
 * gwbp_scatter on the upsampled map, without ever materialising it. */
GWBP_API int gwbp_scatter_upsampled(const gwbp_caps *caps, void *workspace, size_t workspace_bytes,
                           const gwbp_view *view_host, const float *feats, int64_t fs_y, int64_t fs_x, int64_t fs_c,
                           int32_t D, const int32_t *ymap, const int32_t *xmap, float scale_f, float scale_d, float *F,
                           float *d, void *stream);

/* gwbp_scatter over a LOW-RESOLUTION feature map that the reference would first upsample with
 * F.interpolate(mode="bilinear") (lseg variant, backproject.py:110-112; align_corners=False): pixel (y, x) reads
 * h0*(w0*L[y0][x0] + w1*L[y0][x1]) + h1*(w0*L[y1][x0] + w1*L[y1][x1]) with y0 = y0map[y], y1 = min(y0+1, lr_h-1),
 * h1 = ly[y], h0 = 1-h1 (same for x): ATen's UpSampleBilinear2d, computed while the tile's slab is staged.  The maps
 * are device arrays of view.height / view.width entries (engine.bilinear_index builds them like ATen does). */
GWBP_API int gwbp_scatter_bilinear(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                          const float *feats, int64_t fs_y, int64_t fs_x, int64_t fs_c, int32_t D, int32_t lr_h,
                          int32_t lr_w, const int32_t *y0, const float *ly, const int32_t *x0, const float *lx,
                          float scale_f, float scale_d, float *F, float *d, void *stream);

/* Element type of the feature map of the typed scatter entry points below, and of a finished field of the *_typed entry points that
 * read one (gwbp_finalize_typed writes one). */
#define GWBP_MAP_F32 0  /* float32 */
#define GWBP_MAP_F16 1  /* IEEE binary16 */
#define GWBP_MAP_BF16 2 /* bfloat16 (the upper half of a float32) */

/* Typed forms of gwbp_scatter, gwbp_scatter_upsampled, gwbp_scatter_bilinear and gwbp_scatter_tokens: `feats` / `tokens` hold
 * elements of `map_type` and every stride counts ELEMENTS.  An unknown map_type is GWBP_EINVAL, checked before anything else.
 * GWBP_MAP_F32 does exactly what the untyped function does.  A half map (GWBP_MAP_F16 / GWBP_MAP_BF16) is widened to fp32 as it
 * is staged (exact), so F and d equal the untyped function's on the fp32 copy of the map up to the order of the atomic sums
 * (gwbp_scatter_tokens_typed: bit for bit).  Half maps are read natively on these paths only, GWBP_EUNSUPPORTED otherwise:
 *   - gwbp_scatter_typed / _upsampled_typed / _bilinear_typed: D % 128 == 0 and fs_c == 1.  The 256-channel kernel (D % 256 == 0,
 *     no GWBP_FLAG_NARROW_SCATTER) takes any such map.  The 128-channel kernel reads 4 channels per 8-B load and needs fs_x and
 *     fs_y to be multiples of 8 elements and feats 16-B aligned.
 *   - gwbp_scatter_tokens_typed: D % 4 == 0 and D >= 4 (as the untyped function), ts_x and ts_y multiples of 4 elements, tokens
 *     16-B aligned, ts_x >= D.
 * Small D (<= 64), the encoder-fused entry points and maps with fs_c != 1 take float32 only. */
GWBP_API int gwbp_scatter_typed(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                                const void *feats, int32_t map_type, int64_t fs_y, int64_t fs_x, int64_t fs_c, int32_t D,
                                float scale_f, float scale_d, float *F, float *d, void *stream);
GWBP_API int gwbp_scatter_upsampled_typed(const gwbp_caps *caps, void *workspace, size_t workspace_bytes,
                                          const gwbp_view *view_host, const void *feats, int32_t map_type, int64_t fs_y,
                                          int64_t fs_x, int64_t fs_c, int32_t D, const int32_t *ymap, const int32_t *xmap,
                                          float scale_f, float scale_d, float *F, float *d, void *stream);
GWBP_API int gwbp_scatter_bilinear_typed(const gwbp_caps *caps, void *workspace, size_t workspace_bytes,
                                         const gwbp_view *view_host, const void *feats, int32_t map_type, int64_t fs_y,
                                         int64_t fs_x, int64_t fs_c, int32_t D, int32_t lr_h, int32_t lr_w, const int32_t *y0,
                                         const float *ly, const int32_t *x0, const float *lx, float scale_f, float scale_d,
                                         float *F, float *d, void *stream);
GWBP_API int gwbp_scatter_tokens_typed(const gwbp_caps *caps, void *workspace, size_t workspace_bytes,
                                       const gwbp_view *view_host, const void *tokens, int32_t map_type, int64_t ts_y,
                                       int64_t ts_x, int32_t D, const int32_t *ymap, const int32_t *xmap, float scale_f,
                                       float scale_d, float *F, float *d, void *stream);

/* Element type of the label map of gwbp_scatter_labels. */
#define GWBP_LABEL_U8 0  /* uint8_t */
#define GWBP_LABEL_I16 1 /* int16_t */
#define GWBP_LABEL_I32 2 /* int32_t (wider ids: the caller narrows them, sending every id outside [0, num_classes) to -1) */

/* Back-projection of an integer LABEL map (a segmenter's class or instance ids, a binary mask):
 *     F[g, k] += scale_f * sum_p w_g(p) * [L(p) == k],     d[g] += scale_d * sum_p w_g(p)
 * = gwbp_scatter on one_hot(L, num_classes) without the one-hot map: per (Gaussian, tile) record the weights are summed by label
 * and ONE fp32 atomic is added per (record, distinct label); the other columns of the row are never touched.  A label outside
 * [0, num_classes) adds to no column of F but its weight still counts in d (an all-zero one-hot row).  F and d equal
 * gwbp_scatter's on the one-hot map up to the order of the atomic sums.
 * labels[y * ls_y + x * ls_x] (strides in ELEMENTS of label_type); with ymap / xmap (both or neither) a LOW-RESOLUTION map read
 * with PyTorch's nearest rule, pixel (y, x) -> labels[ymap[y] * ls_y + xmap[x] * ls_x] (the index maps of gwbp_scatter_upsampled).
 * F is [N, ldf] fp32 row-major with ldf >= num_classes; d may be NULL (a caller that added d in gwbp_blend_weights_d).
 * GWBP_EINVAL before anything else for an unknown label_type, num_classes <= 0, ldf < num_classes, a NULL F or labels, negative
 * strides, or exactly one of ymap / xmap NULL.  Needs the weight store of the view (gwbp_blend_weights or _d, with or without
 * GWBP_FLAG_NARROW_SCATTER); after gwbp_blend_scatter / gwbp_blend_scatter_encoded / gwbp_blend_tokens the workspace holds none:
 * the call then sets gwbp_stats.overflow bit 2 and leaves F and d untouched. */
GWBP_API int gwbp_scatter_labels(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                                 const void *labels, int32_t label_type, int64_t ls_y, int64_t ls_x, int32_t num_classes,
                                 const int32_t *ymap, const int32_t *xmap, float scale_f, float scale_d, float *F, int64_t ldf,
                                 float *d, void *stream);

/* ---- per-view VOTES of label maps (3-D masks from 2-D masks or masklets) ----------------------------------------------
 * Both entry points add whole votes, per view, to C[g * ldc + k] (fp32 counts, [N, ldc] row-major, ldc >= num_classes) and
 * n[g] (fp32 [N]; may be NULL): C[g, k] += 1 if Gaussian g votes for label k in this view, n[g] += 1 if it votes at all.  A label
 * outside [0, num_classes) is ignored: it counts in n and in no column.  labels, label_type, ls_y, ls_x, ymap, xmap: as
 * gwbp_scatter_labels.  The adds are fp32 atomics (exact up to 2^24 views): several workspaces may add into one C and n at once.
 *
 * gwbp_vote_labels (binary vote): g votes for k if it has at least one weight-store entry (g, p) with w > 0 and L(p) == k, and
 * votes at all if it has one entry with w > 0.  Needs the weight store of the view (gwbp_blend_weights or its _d / _ex / _rgb
 * forms, with or without GWBP_FLAG_NARROW_SCATTER; a pixel weight map's zero or negative values then cast no vote).  seen is the
 * caller's bitset, uint32 [N][ceil((num_classes + 1) / 32)], 4-B aligned, ALL ZERO before the call: the call ORs the view's bits
 * into it and its second kernel adds them to C and n and writes the words back to zero, so one buffer serves every view of one
 * stream (no memset).  After gwbp_blend_scatter / gwbp_blend_scatter_encoded / gwbp_blend_tokens the workspace holds no weight
 * store: the call sets gwbp_stats.overflow bit 2 and adds nothing.
 *
 * gwbp_vote_projected (projection vote): needs gwbp_project (or gwbp_project_camera) of the view only.  A Gaussian with radius > 0
 * whose centre, rounded half to even (x = rint(mx), y = rint(my) of the means2d the projection writes), lies in [0, W) x [0, H)
 * votes for the label at (y, x).  pixel_weights (optional, as the _ex blends, full resolution): a Gaussian whose pixel has a
 * weight that is not > 0 casts no vote.
 *
 * GWBP_EINVAL before anything else for an unknown label_type or pixel weight map, num_classes <= 0, ldc < num_classes, a NULL C,
 * labels or (gwbp_vote_labels) seen, a misaligned seen, negative strides, or exactly one of ymap / xmap NULL. */
GWBP_API int gwbp_vote_labels(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                              const void *labels, int32_t label_type, int64_t ls_y, int64_t ls_x, const int32_t *ymap,
                              const int32_t *xmap, int32_t num_classes, uint32_t *seen, float *C, int64_t ldc, float *n,
                              void *stream);
GWBP_API int gwbp_vote_projected(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                                 const void *labels, int32_t label_type, int64_t ls_y, int64_t ls_x, const int32_t *ymap,
                                 const int32_t *xmap, const gwbp_pixel_weights *pixel_weights, int32_t num_classes, float *C,
                                 int64_t ldc, float *n, void *stream);

/* ---- ASSOCIATION of per-view instance masks (which 3-D group does a mask of a new view continue?) ------------------------
 * Two INTEGER walks of the view's weight store.  Every entry (g, p, w) contributes the fixed-point weight
 *     q = (uint32) rintf(fminf(fmaxf(w, 0), 4) * 1048576)
 * (2^-20 steps, round to nearest and half to even; a NaN or negative stored weight gives 0, a weight above 4 -- possible only
 * with a pixel weight map -- saturates), and every sum of q is an integer sum into int64: the results have the same bits on
 * every run, whatever the order of the atomics.  A record's per-label sum fits uint32 (256 entries of at most 2^22).
 *
 * gwbp_label_overlap:  O[row * ldo + col] += q,  row = L(p) if 0 <= L(p) < num_labels, else num_labels (the ignored pixels
 * have a row of their own, so that a column's sum over all rows is the group's whole weight in this view);  col = group[g] + 1
 * with group int32 [N] (device) in [-1, n_cols - 2], any other value counting as -1: column 0 is "not yet assigned".
 * O is int64 [num_labels + 1, ldo] row-major (device), ldo >= n_cols; the call ADDS (the caller zeroes O).
 *
 * gwbp_label_votes:  V[g * ldv + remap[L(p)]] += q  with remap int32 [num_labels] (device) in [-1, n_cols): a label outside
 * [0, num_labels), a negative remap entry or one >= n_cols adds nothing.  V is int64 [N, ldv] row-major (device), ldv >= n_cols.
 *
 * labels, label_type, ls_y, ls_x, ymap, xmap: as gwbp_scatter_labels.  The caps, the workspace and the view are checked first, as
 * for every call on a view; then, still before any device call, GWBP_EINVAL for an unknown label_type, num_labels <= 0,
 * n_cols <= 0, a leading dimension below n_cols, a NULL labels, group / remap or output, an output that is not 8-B aligned,
 * negative strides, or exactly one of ymap / xmap NULL.  Both need the weight store of the view (gwbp_blend_weights or its _d /
 * _ex / _rgb forms, with or without GWBP_FLAG_NARROW_SCATTER); after gwbp_blend_scatter / gwbp_blend_scatter_encoded /
 * gwbp_blend_tokens the workspace holds none: the call then sets gwbp_stats.overflow bit 2 and leaves its output untouched. */
GWBP_API int gwbp_label_overlap(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                                const void *labels, int32_t label_type, int64_t ls_y, int64_t ls_x, int32_t num_labels,
                                const int32_t *ymap, const int32_t *xmap, const int32_t *group, int32_t n_cols, int64_t *O,
                                int64_t ldo, void *stream);
GWBP_API int gwbp_label_votes(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                              const void *labels, int32_t label_type, int64_t ls_y, int64_t ls_x, int32_t num_labels,
                              const int32_t *ymap, const int32_t *xmap, const int32_t *remap, int32_t n_cols, int64_t *V,
                              int64_t ldv, void *stream);

/* ---- The votes into per-Gaussian SLOT LISTS: label lifts beyond a dense [N, K] -------------------------------------------
 * gwbp_label_votes' walk and arithmetic with a fixed-capacity list of (key, integer sum) slots per Gaussian in place of the
 * dense row: N * (12 * slots + 8) bytes (+ 8 * N with total) whatever the number of ids.
 *
 * The accumulator persists across views and belongs to the caller (device memory):
 *     keys  int32 [N, ld_keys]   -1 = empty; the caller fills it with -1 before the first call
 *     vals  int64 [N, ld_vals]   zero-initialised
 *     spill int64 [N]            zero-initialised
 *     total int64 [N]            zero-initialised; optional, NULL = none
 * with 1 <= slots <= GWBP_SPARSE_MAX_SLOTS = 32 columns in use, unit column stride, and a row stride of its own for keys and for
 * vals (ld_keys, ld_vals >= slots, in elements; columns beyond slots are never touched).
 *
 * The add: for every stored entry (g, p, w) of the view's weight store, c = remap[L(p)] and q as above.  Nothing is added when
 * L(p) lies outside [0, num_labels), when c < 0, or when q == 0.  ANY c >= 0 is a valid key: there is no column count.
 * Otherwise q goes to the slot of row g whose key is c; if no slot has that key, to the first empty slot in index order, which
 * takes the key c for good; if there is neither, to spill[g].  With total, every entry with q != 0 also adds q to total[g],
 * whatever its label: the exact integer denominator of a label field.
 *
 * Invariants (none depends on the order in which the lanes run):
 *   1. a key is never evicted and never appears twice in a row; each slot holds the complete sum of its key over all calls so far;
 *   2. spill[g] is the complete sum of the keys that found no slot; spill[g] > 0 exactly when row g has received more than
 *      `slots` distinct keys with non-zero q: the set of overflowed rows is a function of the input alone;
 *   3. the sum of a row's vals plus spill[g] equals the sum of the dense row gwbp_label_votes would have written;
 *   4. a row without spill holds, as a set, exactly the non-zero entries of that dense row.  Only the slot order depends on the
 *      run; the canonical order removes that: value descending, then key ascending, empties last;
 *   5. in an overflowed row, WHICH `slots` keys hold slots depends on the order of the run: such a row is never exact.
 *
 * The caps, the workspace and the view are checked first; then, before any device call, GWBP_EINVAL for an unknown label_type,
 * num_labels < 1, a NULL remap, slots outside [1, 32], a row stride below slots, a NULL or misaligned keys (4 B), vals or spill
 * (8 B), a misaligned total, byte ranges of keys / vals / spill / total (over the caps' N rows) that overlap each other, exactly
 * one of ymap / xmap NULL, a NULL labels or negative strides.  labels ... xmap, remap and the weight store: as gwbp_label_votes
 * (without one: gwbp_stats.overflow bit 2, the lists untouched). */
#define GWBP_SPARSE_MAX_SLOTS 32
GWBP_API int gwbp_label_votes_sparse(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                                     const void *labels, int32_t label_type, int64_t ls_y, int64_t ls_x, int32_t num_labels,
                                     const int32_t *ymap, const int32_t *xmap, const int32_t *remap, int32_t slots, int32_t *keys,
                                     int64_t ld_keys, int64_t *vals, int64_t ld_vals, int64_t *spill, int64_t *total, void *stream);

/* Bytes of gwbp_scatter_mask_features' slot store per (Gaussian, tile) intersection: four (int32 label, fp32 sum) slots. */
#define GWBP_MASK_SLOT_BYTES 32

/* Back-projection of MASK-POOLED features: a label map L (a segmenter's masks or instances, superpixels) and one embedding per
 * label, table[k * ts_row + c] (k < num_masks, c < D, elements of table_type = GWBP_MAP_*):
 *     F[g, :] += scale_f * sum_p w_g(p) table[L(p), :],     d[g] += scale_d * sum_p w_g(p)
 * = gwbp_scatter on the materialised map table[L] (a zero row where L(p) is outside [0, num_masks): such a pixel adds nothing to
 * F, its weight still counts in d) without the [H, W, D] map, up to the order of the sums.  Per (Gaussian, tile) record the weights
 * are summed by label into up to four (label, sum) slots filed at the record's emit position in `slots`; one wave per Gaussian
 * then multiplies its slots with table rows and updates F[g, :] and d[g] with ONE plain read-modify-write per view -- no atomics,
 * F and d the same bit for bit from run to run.  A record with more than four distinct labels adds the rest with fp32 atomics
 * (the order of those sums varies) and adds 1 to *n_spilled (device, optional).
 * labels, label_type, ls_y, ls_x, ymap, xmap: as gwbp_scatter_labels.  table: 16-B aligned (fp32) or 8-B aligned (fp16 / bf16),
 * ts_row >= D and a multiple of 4; a half table is widened as it is read (F equals that of the fp32 table).  F is [N, D] fp32
 * dense and 16-B aligned, D a positive multiple of 4; d may be NULL (a caller that added d in gwbp_blend_weights_d).
 * slots: caller-owned device scratch of at least GWBP_MASK_SLOT_BYTES * caps->isect_cap bytes, 16-B aligned, only used during
 * the call's kernels (one buffer per stream).
 * GWBP_EINVAL before anything else for an unknown label or table type, num_masks <= 0, a D that is no positive multiple of 4,
 * bad map or table arguments, exactly one of ymap / xmap NULL, a NULL or misaligned F, or missing / short slots.  Needs the
 * weight store of the view (as gwbp_scatter_labels); after gwbp_blend_scatter / gwbp_blend_scatter_encoded / gwbp_blend_tokens
 * the call sets gwbp_stats.overflow bit 2 and leaves F and d untouched. */
GWBP_API int gwbp_scatter_mask_features(const gwbp_caps *caps, void *workspace, size_t workspace_bytes,
                                        const gwbp_view *view_host, const void *labels, int32_t label_type, int64_t ls_y,
                                        int64_t ls_x, const int32_t *ymap, const int32_t *xmap, const void *table,
                                        int32_t table_type, int64_t ts_row, int32_t num_masks, int32_t D, float scale_f,
                                        float scale_d, float *F, float *d, void *slots, size_t slots_bytes,
                                        uint32_t *n_spilled, void *stream);

/* Forward render (what rasterization() returns): out[p,:] = sum_g w_g(p) * colors[g,:], out is [H,W,D]. */
GWBP_API int gwbp_render(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                const float *colors, int32_t D, float *out, void *stream);

/* gwbp_render with a typed colour table and a typed output.  `color_type` (GWBP_MAP_F32 / _F16 / _BF16) is the element type of colors,
 * ldc >= D its row stride in ELEMENTS (the untyped function reads a dense table: ldc = D); `out_type` is the element type of the dense
 * [H, W, D] out.  An unknown type code is GWBP_EINVAL, checked before anything else; then the caps, the workspace and the view as in
 * gwbp_render; a stride below D, a pointer that is not aligned to its element (4 B, 2 B) or a half out that is colors are GWBP_EINVAL
 * before any HIP call.  GWBP_MAP_F32 / GWBP_MAP_F32 does exactly what gwbp_render does (which is a call of this one).
 * A half table is read as stored: the kernels keep the bits a load landed and widen them -- exact -- where they are multiplied, so out
 * has the BITS gwbp_render gives on the fp32 copy of the table, NaN positions included, and no such copy is made.  A half out is the
 * fp32 sum rounded ONCE to nearest even (gwbp_finalize_typed's rule): the bits of converting the fp32 out.  The kernel that holds four
 * or eight channels per lane takes D >= 128, D % 4 == 0, table rows that are 16-B (fp32) / 8-B (half) aligned at a stride that is a
 * multiple of 4 elements, and an out aligned likewise; every other layout takes the two-channel kernel, with the same bits. */
GWBP_API int gwbp_render_typed(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                               const void *colors, int32_t color_type, int64_t ldc, int32_t D, void *out, int32_t out_type,
                               void *stream);

/* Forward render for 1..32 channels (RGB, RGB+D, depth; round 5: the 16-d compressed field) straight from the sorted tile
 * lists (needs gwbp_project + gwbp_bin_sort of the same view, not the weight store): the render the reference feeds to its
 * 2-D feature network (backproject.py:89-100), compares in utils.test_proper_pruning (utils.py:316-340) and scores per frame
 * in segment_compressed.py:154-165.  alphas[H*W] optional. */
GWBP_API int gwbp_render_pixels(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                       const float *colors, int32_t D, float *out, float *alphas, void *stream);

/* gwbp_render_pixels with a typed colour table: color_type, ldc and the checks as in gwbp_render_typed; out and alphas stay fp32.  A
 * half row is read by the thread that stages its Gaussian -- 8-B loads of four elements where the table is 8-B aligned and ldc a
 * multiple of 4, 2-B loads otherwise -- and widened where it enters LDS: the bits of gwbp_render_pixels on the fp32 copy. */
GWBP_API int gwbp_render_pixels_typed(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                                      const void *colors, int32_t color_type, int64_t ldc, int32_t D, float *out, float *alphas,
                                      void *stream);

/* Backward of gwbp_render_pixels for an fp32 table (gsplat's rasterize_to_pixels_bwd): needs gwbp_project (or gwbp_project_camera) +
 * gwbp_bin_sort of the same view in the workspace, not the weight store, and writes nothing into the workspace.
 *   colors float [N, ldc], 1 <= D <= 32, ldc >= D: the table that was rendered.
 *   v_out float [H, W, D] (dense), v_alpha float [H, W] or NULL: the gradient that reaches the render and its alpha map.
 *   v_g2d float [N, 6], ADDED INTO: d / d(mx, my, ca, cb, cc, o) of each projected record -- the 2-D mean, the conic and the opacity the
 *          blend read, which under the antialiased mode already holds the compensation.  A pair whose o exp(-sigma) was clamped at
 *          0.999 adds nothing here (its alpha does not move), as in gsplat.
 *   v_colors float [N, D] (dense) or NULL, ADDED INTO: d / d(colors).
 * The caller zeroes the outputs.  The kernel replays the forward walk with the render's own expressions (the same valid pairs, the
 * same T bit for bit), then walks each tile's list back to front; each record's sums over a tile are added with one float atomic per
 * value, in an order that is not fixed: the results are NOT bit-reproducible from run to run.
 * After the caps, the workspace and the view: D outside [1, 32], a null colors, v_out or v_g2d, ldc < D or a pointer that is not 4-B
 * aligned are GWBP_EINVAL before any HIP call. */
GWBP_API int gwbp_render_pixels_backward(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                                         const float *colors, int64_t ldc, int32_t D, const float *v_out, const float *v_alpha,
                                         float *v_colors, float *v_g2d, void *stream);

/* The geometry half of that backward for tables of up to 128 channels: v_g2d alone, from the same workspace state (gwbp_project +
 * gwbp_bin_sort of the view; the weight store is not read and nothing is written into the workspace).
 *   colors float [N, ldc], 1 <= D <= 128, ldc >= D; v_out float [H, W, D] (dense); v_alpha float [H, W] or NULL.
 *   v_g2d float [N, 6], ADDED INTO: as gwbp_render_pixels_backward defines it, with the same valid pairs and the same clamp rule.
 * The channels enter d loss / d alpha of a (pixel, record j) pair only through m_j = <colors_j, v_out_p>:
 *     v_alpha_j = T_j m_j - B_j / (1 - alpha_j) + T_final v_alpha_p / (1 - alpha_j),  B_j = sum over the records k behind j of alpha_k T_k m_k,
 * so a pixel carries one scalar beside its v_out row.  d / d(colors) is NOT computed: it is gwbp_scatter of v_out over the weight
 * store that a wide forward render (gwbp_blend_weights + gwbp_render) leaves.  Sums are float atomics in an order that is not fixed.
 * After the caps, the workspace and the view: D outside [1, 128], a null colors, v_out or v_g2d, ldc < D or a pointer that is not 4-B
 * aligned are GWBP_EINVAL before any HIP call. */
GWBP_API int gwbp_render_dots_backward(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                                       const float *colors, int64_t ldc, int32_t D, const float *v_out, const float *v_alpha,
                                       float *v_g2d, void *stream);

/* Backward of gwbp_project / gwbp_project_camera (gsplat's fully_fused_projection_bwd, and the view-matrix gradient with it): needs
 * the projection of the same view (same camera_model, rasterize_mode and Gaussians) in the workspace -- a row is visible when its
 * record there has radius > 0 -- and writes nothing into the workspace.
 *   means, quats, scales, opacities: what was projected.  v_g2d float [N, 6]: d / d(mx, my, ca, cb, cc, o) of each projected record,
 *          as gwbp_render_pixels_backward leaves it.
 *   v_means [N, 3], v_quats [N, 4], v_scales [N, 3], v_opacities [N], float, each may be NULL: WRITTEN, not added into.  The chain is
 *          evaluated in float64 from the stored float32 inputs (the forward is recomputed; the filed float32 conic is not read) and each
 *          value rounded once.  The function differentiated is the projection's: the quaternion normalised inside, the pinhole clamp of
 *          x/z and y/z inside the Jacobian passing no gradient where it binds, the eps2d low-pass, and under the antialiased mode the
 *          compensation (zero gradient where det(S) / det(S + eps2d I) is not positive).  A culled row gets zeros and is not evaluated.
 *   v_viewmat double [12] or NULL: d / d(viewmat[:3, :3]) row-major, then d / d(viewmat[:3, 3]), summed over the visible rows without
 *          atomics in a fixed order (wave, block, then the blocks in order): the same inputs give the same bits.  It needs
 *   scratch double [gwbp_project_backward_blocks(N), 12], which the call overwrites.
 * After the caps, the workspace and the view: an unknown camera model or rasterize mode, a null means / quats / scales / opacities /
 * v_g2d, every output null, v_viewmat without scratch, quats or v_quats not 16-B aligned, v_viewmat or scratch not 8-B aligned or any
 * other pointer not 4-B aligned are GWBP_EINVAL before any HIP call. */
GWBP_API int gwbp_project_backward(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                                   int32_t camera_model, int32_t rasterize_mode, const float *means, const float *quats,
                                   const float *scales, const float *opacities, const float *v_g2d, float *v_means, float *v_quats,
                                   float *v_scales, float *v_opacities, double *v_viewmat, double *scratch, void *stream);

/* Rows of gwbp_project_backward's scratch for n_gaussians Gaussians (one per workgroup of 256: ceil(n / 256)), or GWBP_EINVAL. */
GWBP_API int gwbp_project_backward_blocks(int64_t n_gaussians);

/* gsplat spherical_harmonics + "+0.5, clamp at 0": coeffs[N,K,3] (K >= (degree+1)^2, degree <= 3), view directions
 * means - campos_host[3]; out[N,3].  What rasterization(..., sh_degree=3) does before rasterising (backproject.py:99). */
GWBP_API int gwbp_sh_colors(int64_t N, int32_t degree, int32_t K, const float *means, const float *coeffs,
                   const float *campos_host, float *out, void *stream);

/* The same colours from a coefficient row that is stored in two tables, and their backward (csrc/sh.hip, csrc/sh_math.h): what a
 * training step evaluates from features_dc and features_rest as they are stored.
 * Coefficient k of Gaussian i is head[i][k] for k < K_head and tail[i][k - K_head] behind; both tables are contiguous float32
 * [N, K_*, 3]; tail == NULL with K_tail == 0 is the single-table call.  Rows from (degree + 1)^2 on are not used.
 * gwbp_sh_eval  out[N, 3]: the bits gwbp_sh_colors gives on the concatenated table.
 * gwbp_sh_eval_backward  from v_colors[N, 3] = d loss / d out, WRITES (each output may be NULL, not all of them):
 *     v_head[N, K_head, 3], v_tail[N, K_tail, 3]: b_k(dir) v_c for k < (degree + 1)^2, exact +0 in the rows behind; a channel passes
 *         v_c where the forward's own float32 pre-clamp value r has r + 0.5f >= 0 (torch's clamp_min rule; a NaN passes nothing);
 *     v_means[N, 3]: the gradient through the view direction dir = d / max(|d|, 1e-12), d = mean - campos:
 *         (v_dir - dir <dir, v_dir>) / |d| where |d| > 1e-12 and v_dir 1e12 otherwise; zeros at degree 0.
 * It recomputes the forward from its inputs.  One thread owns a Gaussian, there are no atomics: the same bits every run.
 * GWBP_EINVAL before any HIP call: N outside [0, 2^31 - 1], degree outside 0..3, K_head < 1, K_tail < 0, K_head + K_tail below
 * (degree + 1)^2 or above GWBP_SH_MAX_K, tail == NULL with K_tail > 0, a null campos_host, a null required array where N > 0, every
 * backward output null, an array that is not 4-B aligned, an output that is one of the inputs or another output. */
#define GWBP_SH_MAX_K 16
GWBP_API int gwbp_sh_eval(int64_t N, int32_t degree, int32_t K_head, int32_t K_tail, const float *means, const float *head,
                          const float *tail, const float *campos_host, float *out, void *stream);
GWBP_API int gwbp_sh_eval_backward(int64_t N, int32_t degree, int32_t K_head, int32_t K_tail, const float *means, const float *head,
                                   const float *tail, const float *campos_host, const float *v_colors, float *v_head, float *v_tail,
                                   float *v_means, void *stream);

/* The same pair for a camera centre that lives on the device (a pose that is trained with the Gaussians): campos is a DEVICE pointer
 * to three floats, loaded by the kernels and never read on the host.  For the same three values gwbp_sh_eval_dev gives gwbp_sh_eval's
 * bits, and gwbp_sh_eval_backward_dev gives gwbp_sh_eval_backward's v_head, v_tail and v_means bits.  It adds
 *   v_campos double [3] or NULL: d loss / d campos = minus the sum over the rows of their float32 v_means values (the direction is
 *          mean - campos), each widened to double and added without atomics in a fixed order (wave, block, then the blocks in
 *          order): the same inputs give the same bits; exact +0 at degree 0 and at N = 0.  Where N > 0 it needs
 *   scratch double [gwbp_sh_eval_backward_blocks(N), 3], which the call overwrites.
 * GWBP_EINVAL before any HIP call: as for the pair above (campos in the place of campos_host, and 4-B aligned), every one of the four
 * outputs null, v_campos without scratch where N > 0, v_campos or scratch not 8-B aligned, an output or the scratch that is one of the
 * inputs or another output. */
GWBP_API int gwbp_sh_eval_dev(int64_t N, int32_t degree, int32_t K_head, int32_t K_tail, const float *means, const float *head,
                              const float *tail, const float *campos, float *out, void *stream);
GWBP_API int gwbp_sh_eval_backward_dev(int64_t N, int32_t degree, int32_t K_head, int32_t K_tail, const float *means,
                                       const float *head, const float *tail, const float *campos, const float *v_colors,
                                       float *v_head, float *v_tail, float *v_means, double *v_campos, double *scratch, void *stream);
/* Rows of gwbp_sh_eval_backward_dev's scratch for n_gaussians Gaussians (one per workgroup of 256: ceil(n / 256)), or GWBP_EINVAL. */
GWBP_API int gwbp_sh_eval_backward_blocks(int64_t n_gaussians);

/* ---- fused entry points --------------------------------------------------------------------------------- */

/* project -> bin_sort -> blend_weights -> scatter for one view: the per-view body of
 * create_feature_field_lseg (backproject.py:115-151) in one call, one blend instead of two.  Pinhole camera, classic
 * rasterize mode only: other camera settings go through gwbp_project_camera and the stage entry points. */
GWBP_API int gwbp_backproject_view(const gwbp_caps *caps, void *workspace, size_t workspace_bytes,
                          const gwbp_view *view_host, const float *means, const float *quats, const float *scales,
                          const float *opacities, const float *feats, int64_t fs_y, int64_t fs_x, int64_t fs_c,
                          int32_t D, float scale_f, float scale_d, float *F, float *d, void *stream);

/* backproject_compressed.py:127: out[y, x, :] = feats[y, x, :] @ encoder, encoder [K, n_out] row-major, n_out <= 16,
 * K % 16 == 0, feats[y*fs_y + x*fs_x + c] (channel-contiguous pixels, 16-B aligned), out [H, W, n_out] dense.  The map is
 * read once at HBM rate; exact fp32 (v_mfma_f32_16x16x4_f32 = a k-ordered fmaf chain).  workgroups: 0 = as many as
 * stream fastest alone (6.0 TB/s); a caller that overlaps the encoder with latency-bound kernels passes one per CU. */
GWBP_API int gwbp_encode_map(const float *feats, int64_t fs_y, int64_t fs_x, int32_t height, int32_t width, int32_t K,
                    const float *encoder, int32_t n_out, float *out, int32_t workgroups, void *stream);

/* backproject.py:63,166-169: out = normalize(F / (1e-12 + d)), NaN -> 0.  out may alias F. */
GWBP_API int gwbp_finalize(int64_t N, int32_t D, const float *F, const float *d, float *out, void *stream);

/* gwbp_finalize with a typed OUTPUT: out holds N x D elements of `out_type` (GWBP_MAP_F32 / _F16 / _BF16), dense.  An unknown out_type
 * is GWBP_EINVAL, checked before anything else; an out that is not aligned to its element is GWBP_EINVAL before any HIP call.
 * GWBP_MAP_F32 does exactly what gwbp_finalize does (which is a call of this one).  For a half type the fp32 value gwbp_finalize
 * computes (NaN -> 0 included) is rounded ONCE, to nearest even, subnormal fp16 results kept: out equals the fp32 result converted by
 * torch's .to(dtype), bit for bit.  F and d stay fp32.  A half out cannot alias F (GWBP_EINVAL). */
GWBP_API int gwbp_finalize_typed(int64_t N, int32_t D, const float *F, const float *d, void *out, int32_t out_type, void *stream);

/* Inner-product k-nearest-neighbour search on a finished field (faiss IndexFlatIP.search; the reference's transfer_affordance,
 * affordance_transfer/demo_affordance_transfer.py:1377-1396): for every query row Q[g * ldq + 0..D-1], g < N, the k source rows
 * S[j * lds_ + 0..D-1], j < M, of largest inner product.  idx[N, k] (int32) and score[N, k] (fp32) are dense; each row is sorted
 * by score descending, then index ascending.  1 <= k <= 32, k <= M < 2^31, D >= 1, ldq >= D, lds_ >= D (strides in floats: the
 * padded storage of a field goes in as it is).  Scores and selection are fused in one kernel: no score reaches global memory,
 * and the call needs no workspace.
 * Arithmetic: every score is one chain of fp32 fused multiply-adds over the D index in an order that depends only on D (the fp32
 * matrix cores; no reduced-precision operand): results do not depend on a row's position in Q or S, on N, M, k or the launch;
 * identical source rows tie bit for bit and come in index order; a zero query row scores +0 against every finite source and
 * returns 0 .. k-1.  A NaN score (a NaN, or 0 x inf, in either row) orders after every number, NaNs among themselves by index.
 * Rows whose addresses and strides are 16-B aligned are read with 16-B loads, others element by element (same results).
 * GWBP_EINVAL before any HIP call: N < 0, M < 1, D < 1, k outside [1, 32], k > M, a stride below D, a null or misaligned pointer. */
GWBP_API int gwbp_knn_search(int64_t N, int32_t M, int32_t D, int32_t k, const float *Q, int64_t ldq, const float *S,
                             int64_t lds_, int32_t *idx, float *score, void *stream);

/* gwbp_knn_search with a typed QUERY field Q: `field_type` (GWBP_MAP_F32 / _F16 / _BF16) is the element type of that one operand and its row stride counts
 * ELEMENTS.  An unknown field_type is GWBP_EINVAL, checked before anything else; a field pointer that is not aligned to its element
 * (4 B, 2 B) is GWBP_EINVAL before any HIP call, as are the untyped function's own invalid cases.  GWBP_MAP_F32 does exactly what
 * the untyped function does (which is a call of this one).  A half field is widened to fp32 as it is loaded or staged -- exact --
 * so every result has the BITS the untyped function gives on the fp32 copy of the field, and no such copy is made.  Half rows whose
 * address is 8-B aligned and whose stride is a multiple of 4 elements move with one 8-B load per four channels, others element by
 * element, with the same bits. The sources S, idx and score stay fp32 / int32. */
GWBP_API int gwbp_knn_search_typed(int64_t N, int32_t M, int32_t D, int32_t k, const void *Q, int32_t field_type, int64_t ldq,
                                   const float *S, int64_t lds_, int32_t *idx, float *score, void *stream);

/* The majority label of each row of gwbp_knn_search's idx[N, k]: label_out[g] = the most frequent of labels[idx[g, 0..k-1]], the
 * SMALLEST label among equally frequent ones (np.bincount(row).argmax()).  labels: int32 [M]; a label outside [0, num_classes)
 * and an index outside [0, M) are ignored; a row with nothing left gets -1.  counts (optional, may be NULL): int32
 * counts[g * ldc + c], c < num_classes, the row's histogram (overwritten).
 * GWBP_EINVAL before any HIP call: N < 0, M < 1, k outside [1, 32], num_classes <= 0, ldc < num_classes, a null pointer. */
GWBP_API int gwbp_knn_vote(int64_t N, int32_t M, int32_t k, const int32_t *idx, const int32_t *labels, int32_t num_classes,
                           int32_t *label_out, int32_t *counts, int64_t ldc, void *stream);

/* ---- Spatial neighbours: exact Euclidean k-NN of 3-D points on a uniform grid (the reference's knn(),
 * f3dgs/utils_simple_trainer.py:141-145: sklearn NearestNeighbors on a host copy) -------------------------------------------------
 * The grid: cubic cells of edge cell_size over a box that starts at (lo_x, lo_y, lo_z), nx x ny x nz cells, x fastest.  A point's
 * cell along an axis is floorf((x - lo) / cell_size) clamped to [0, n - 1]: the border cells extend to infinity.  The result of the
 * search does not depend on the grid, only its cost does.
 * The three calls of one search, with the caller's stable sort of the keys between the first two:
 *   gwbp_spatial_cell_keys  keys[i] = the linear cell of points[i * ldp + 0..2] (int32); a point with a non-finite coordinate gets
 *                           the key nx * ny * nz, which sorts last and belongs to no cell.
 *   gwbp_spatial_build      from the keys in ascending order (sorted_keys[n]) and the permutation that sorts them (perm[n], int64):
 *                           sorted[i] = (x, y, z, original index as int32 bits) of point perm[i] (float [n, 4], 16-B aligned), and
 *                           cell_start[c], c <= n_cells = nx * ny * nz (int32 [n_cells + 1]): the first sorted position whose key
 *                           is >= c.  No atomics.
 *   gwbp_spatial_knn        for every query row queries[g * ldq + 0..2], g < q, the k points of smallest distance: idx[q, k] (int32,
 *                           original indices) and dist[q, k] (fp32), dense, each row sorted by distance ascending, then index
 *                           ascending.  order[q] (int64): the order in which lanes take the queries -- a permutation of 0 .. q-1,
 *                           by ascending cell key of the queries for speed (for queries == points: perm).
 * Arithmetic: squared distance is fmaf(dz, dz, fmaf(dy, dy, dx * dx)) with dx = p.x - q.x in fp32; dist is its correctly rounded
 * sqrtf.  The search is exact for that expression: ties by index, results independent of the grid and of the launch, no atomics,
 * two runs give the same bits.  A non-finite point is nobody's neighbour; a non-finite query gets idx -1 and dist NaN; a query
 * with fewer than k finite points gets idx -1 and dist +inf in the tail.  1 <= k <= 32, k <= n < 2^31; 1 <= nx, ny, nz <= 1024,
 * nx * ny * nz <= 2^24; cell_size finite and >= GWBP_SPATIAL_MIN_CELL; row strides (in floats) >= 3.
 * GWBP_EINVAL before any HIP call: a size, k, grid dimension, cell size or stride outside these, a null or misaligned pointer. */
#define GWBP_SPATIAL_MAX_DIM 1024
#define GWBP_SPATIAL_MAX_CELLS (1 << 24)
#define GWBP_SPATIAL_MIN_CELL 1e-30f
GWBP_API int gwbp_spatial_cell_keys(int64_t n, const float *points, int64_t ldp, float lo_x, float lo_y, float lo_z,
                                    float cell_size, int32_t nx, int32_t ny, int32_t nz, int32_t *keys, void *stream);
GWBP_API int gwbp_spatial_build(int64_t n, const float *points, int64_t ldp, const int32_t *sorted_keys, const int64_t *perm,
                                int64_t n_cells, float *sorted, int32_t *cell_start, void *stream);
GWBP_API int gwbp_spatial_knn(int64_t n, const float *sorted, const int32_t *cell_start, float lo_x, float lo_y, float lo_z,
                              float cell_size, int32_t nx, int32_t ny, int32_t nz, int64_t q, const float *queries, int64_t ldq,
                              const int64_t *order, int32_t k, int32_t *idx, float *dist, void *stream);

/* The average of a field over each row's neighbour list: out[g * ldo + c] = (sum over the valid j, in the list's order, of
 * features[idx[g * k + j] * ldf + c]) / (the number of valid j), g < n, c < D, fp32.  An index outside [0, m) is skipped (the -1 of
 * gwbp_spatial_knn); a row with no valid index is zero.  features is read in place at any row stride ldf >= D; out is another
 * buffer, ldo >= D.  Rows whose addresses and strides are 16-B aligned move with 16-B loads and stores (same results).  No atomics.
 * GWBP_EINVAL before any HIP call: n < 0, m < 1, D < 1, k outside [1, 32], a stride below D, a null or misaligned pointer,
 * out == features. */
GWBP_API int gwbp_neighbor_mean(int64_t n, int64_t m, int32_t D, int32_t k, const int32_t *idx, const float *features,
                                int64_t ldf, float *out, int64_t ldo, void *stream);

/* gwbp_neighbor_mean with a typed field `features`: `field_type` (GWBP_MAP_F32 / _F16 / _BF16) is the element type of that one operand and its row stride counts
 * ELEMENTS.  An unknown field_type is GWBP_EINVAL, checked before anything else; a field pointer that is not aligned to its element
 * (4 B, 2 B) is GWBP_EINVAL before any HIP call, as are the untyped function's own invalid cases.  GWBP_MAP_F32 does exactly what
 * the untyped function does (which is a call of this one).  A half field is widened to fp32 as it is loaded or staged -- exact --
 * so every result has the BITS the untyped function gives on the fp32 copy of the field, and no such copy is made.  Half rows whose
 * address is 8-B aligned and whose stride is a multiple of 4 elements move with one 8-B load per four channels, others element by
 * element, with the same bits. out stays fp32. */
GWBP_API int gwbp_neighbor_mean_typed(int64_t n, int64_t m, int32_t D, int32_t k, const int32_t *idx, const void *features,
                                      int32_t field_type, int64_t ldf, float *out, int64_t ldo, void *stream);

/* gwbp_neighbor_mean_typed with a typed OUTPUT: `out_type` (GWBP_MAP_*) is the element type of out and ldo counts ITS elements.  A
 * half out is the fp32 quotient rounded ONCE to nearest even (gwbp_finalize_typed's rule): the bits of converting the fp32 out.  An
 * unknown out_type is GWBP_EINVAL beside an unknown field_type, before anything else; an out that is not aligned to its element, or
 * that is the features (whatever its type), is GWBP_EINVAL before any HIP call.  gwbp_neighbor_mean_typed is a call of this function
 * with GWBP_MAP_F32. */
GWBP_API int gwbp_neighbor_mean_out_typed(int64_t n, int64_t m, int32_t D, int32_t k, const int32_t *idx, const void *features,
                                          int32_t field_type, int64_t ldf, void *out, int32_t out_type, int64_t ldo, void *stream);

/* ---- Radius components: which points form one object (DBSCAN with a deterministic border rule; PCL's Euclidean cluster extraction
 * at min_points = 1) on the grid of the spatial search above ------------------------------------------------------------------------
 * sorted / cell_start / the grid arguments: what gwbp_spatial_cell_keys + the caller's stable sort + gwbp_spatial_build made of
 * points[n, 3].  group (optional, may be NULL: every point in group 0): int32 [n] in the points' ORIGINAL order.  The contract:
 *   d2(p, q) = fmaf(dz, dz, fmaf(dy, dy, dx * dx)), dx = p.x - q.x in fp32 (gwbp_spatial_knn's); r2 = the caller's fp32 product
 *     radius * radius; a point is LIVE when its coordinates are finite and its group is >= 0;
 *   i and j are NEIGHBOURS when both are live, group[i] == group[j] and d2 <= r2 (a point is its own neighbour);
 *   count[i] = the number of neighbours of i; i is CORE when count[i] >= min_points;
 *   two core points are in one COMPONENT when a chain of core points, each a neighbour of the next, joins them;
 *   a live non-core point with a core neighbour is a BORDER point of the component of its nearest core neighbour by (d2, index).
 * The results are pure functions of the points, the groups, r2 and min_points: they do not depend on the grid, on the launch or on
 * the order in which lanes run, and two runs give the same bits.
 *   gwbp_radius_count        count[g] (int32 [q]) = min(cap, the number of points with d2 <= r2 to query row queries[g * ldq + 0..2]
 *                            whose group equals the query's), g < q.  query_group (optional: every query in group 0): int32 [q].  A
 *                            non-finite query or one with a negative group gets 0.  order[q]: as for gwbp_spatial_knn.  The walk of
 *                            a query ends once its count has reached cap (cap >= 1; INT32_MAX: the full count).  visited (optional):
 *                            int32 [q], the number of points whose distance the query's lane computed.
 *   gwbp_radius_union        for every core point i (count[i] >= min_points) and every core neighbour j < i: unite(i, j) in
 *                            parent[n] (int32, the identity on entry), a union-find by index: a hook stores a smaller index over a
 *                            root with an agent-scope compare-and-swap, so parent[v] <= v always, a find walks strictly decreasing
 *                            indices, and a component's final root is its smallest member.  No lane waits for another.  count: as
 *                            written by gwbp_radius_count for queries == points, order == perm, query_group == group, cap >=
 *                            min_points.  The roots are read by gwbp_components_flatten, a launch of its own.
 *   gwbp_radius_attach       attach[i] (int32 [n]) = for a live non-core point (0 < count[i] < min_points) its nearest core
 *                            neighbour by (d2, index), -1 if it has none; -1 for every other point.
 *   gwbp_components_flatten  root[i] (int32 [n]) = the root of i for a core point, of attach[i] for a point with attach[i] >= 0
 *                            (attach may be NULL: no border points), else -1.
 * status (int32 [1], zero on entry): set to 1 if a loop of the union-find reached its trip cap of n + 1, which the invariant above
 * rules out; the caller reads it after gwbp_components_flatten.
 * 1 <= n < 2^31; r2 >= 0 (+inf allowed: everything is within reach); min_points, cap >= 1; the grid as for gwbp_spatial_knn.
 * GWBP_EINVAL before any HIP call: a size, r2, cap, min_points, grid dimension, cell size or stride outside these, a null or
 * misaligned pointer. */
GWBP_API int gwbp_radius_count(int64_t n, const float *sorted, const int32_t *cell_start, float lo_x, float lo_y, float lo_z,
                               float cell_size, int32_t nx, int32_t ny, int32_t nz, const int32_t *group, float r2, int64_t q,
                               const float *queries, int64_t ldq, const int64_t *order, const int32_t *query_group, int32_t cap,
                               int32_t *count, int32_t *visited, void *stream);
GWBP_API int gwbp_radius_union(int64_t n, const float *sorted, const int32_t *cell_start, float lo_x, float lo_y, float lo_z,
                               float cell_size, int32_t nx, int32_t ny, int32_t nz, const int32_t *group, float r2,
                               const int32_t *count, int32_t min_points, int32_t *parent, int32_t *status, void *stream);
GWBP_API int gwbp_radius_attach(int64_t n, const float *sorted, const int32_t *cell_start, float lo_x, float lo_y, float lo_z,
                                float cell_size, int32_t nx, int32_t ny, int32_t nz, const int32_t *group, float r2,
                                const int32_t *count, int32_t min_points, int32_t *attach, void *stream);
GWBP_API int gwbp_components_flatten(int64_t n, const int32_t *count, int32_t min_points, const int32_t *attach, int32_t *parent,
                                     int32_t *root, int32_t *status, void *stream);

/* ---- Regions: the connected components of a neighbour list whose edges pass a cosine threshold (region growing on the feature
 * field over the spatial k-NN graph) --------------------------------------------------------------------------------------------------
 * features[n, D]: fp32, row i at features + i * ldf, ldf >= D.  idx[n, k]: int32, dense; an entry < 0 or >= n is NO NEIGHBOUR; an
 * entry == i is allowed and ignored by the union.  dist[n, k] (optional, may be NULL): fp32, gwbp_spatial_knn's distances for the
 * same list.  group[n] (optional, may be NULL: every point in group 0): int32.  The contract:
 *   dot(i, j) = sum_c F[i, c] * F[j, c] and sq(i) = dot(i, i) are each ONE fixed arrangement of fp32 operations that depends on D
 *     alone: lane l of 64 owns the channels 256 s + 4 l + e (s = 0, 1, ...; e = 0 .. 3; those < D) and runs acc = fmaf(a, b, acc)
 *     from acc = +0 in the order (s, e); the 64 partial sums are then combined by the butterfly p_l = p_l + p_(l xor o) for o = 1,
 *     2, 4, 8, 16, 32.  (A channel >= D may be skipped or enter as a product of zeros: the bits are the same, since an accumulator
 *     that starts at +0 never becomes -0.)  The arrangement is symmetric -- dot(i, j) has the bits of dot(j, i), and sq(j) has the
 *     same bits whichever row's wave computes it -- and independent of n, k, the row's position, ldf, the alignment and the launch;
 *   norm(i) = sqrtf(sq(i)), correctly rounded; row i is FEATURE-LIVE when sq(i) is finite and norm(i) >= 1e-12f (F.normalize's
 *     epsilon; a zero row and a row with a NaN or an infinity are dead);
 *   sim[i, c] = dot(i, j) / (norm(i) * norm(j)), j = idx[i, c]: one fp32 multiply and one correctly rounded divide; NaN when j is
 *     no neighbour or either row is not feature-live.  (sim of two bit-identical rows is whatever this gives, not always 1.)
 *   live(i) = row i is feature-live and group[i] >= 0;
 *   i -- j is an EDGE when j = idx[i, c] for some c (or i = idx[j, c]), i != j, both are live, group[i] == group[j], sim[i, c] >=
 *     sim_min (NaN fails), and, when a cut is given (dist not NULL and max_dist < +inf), dist[i, c] <= max_dist;
 *   the COMPONENTS are those of the live points under the edges (a live point without an edge is a component of one); a
 *     component's root is its smallest member; everything else gets root -1.
 * The results are pure functions of (features, idx, dist, group, sim_min, max_dist), whatever the order in which lanes run; two
 * runs give the same bits.
 *   gwbp_neighbor_similarity  sim[n, k] (fp32, dense) and live[n] (int32 0 / 1: FEATURE-live only).  One wave per row; rows whose
 *                             addresses and stride are 16-B aligned are read with 16-B loads, others element by element, with the
 *                             same chains and bits.  No atomics.
 *   gwbp_edge_union           for every edge found in row i's list: unite(i, j) in parent[n] (int32, the identity on entry), the
 *                             union-find by index of gwbp_radius_union; count[i] (int32 [n]) = live[i] && group[i] >= 0.  sim and
 *                             live: as written by gwbp_neighbor_similarity for the same idx.  gwbp_components_flatten(n, count, 1,
 *                             NULL, parent, root, status) then reads the roots, in a launch of its own.  status: as above.
 * 1 <= n < 2^31, 1 <= D <= GWBP_REGIONS_MAX_D, 1 <= k <= GWBP_REGIONS_MAX_K, ldf >= D; sim_min is not NaN; max_dist >= 0 or +inf.
 * Every array is a buffer of its own: an output (sim, live; count, parent, status) is none of the call's inputs and no other output.
 * GWBP_EINVAL before any HIP call: a size, stride, sim_min or max_dist outside these, a null required pointer, a misaligned
 * pointer (4-B), an output array that is an input array or another output. */
#define GWBP_REGIONS_MAX_D 2048
#define GWBP_REGIONS_MAX_K 64
GWBP_API int gwbp_neighbor_similarity(int64_t n, int32_t D, int32_t k, const int32_t *idx, const float *features, int64_t ldf,
                                      float *sim, int32_t *live, void *stream);

/* gwbp_neighbor_similarity with a typed field `features` (own and neighbour rows): `field_type` (GWBP_MAP_F32 / _F16 / _BF16) is the element type of that one operand and its row stride counts
 * ELEMENTS.  An unknown field_type is GWBP_EINVAL, checked before anything else; a field pointer that is not aligned to its element
 * (4 B, 2 B) is GWBP_EINVAL before any HIP call, as are the untyped function's own invalid cases.  GWBP_MAP_F32 does exactly what
 * the untyped function does (which is a call of this one).  A half field is widened to fp32 as it is loaded or staged -- exact --
 * so every result has the BITS the untyped function gives on the fp32 copy of the field, and no such copy is made.  Half rows whose
 * address is 8-B aligned and whose stride is a multiple of 4 elements move with one 8-B load per four channels, others element by
 * element, with the same bits. sim and live stay fp32 / int32. */
GWBP_API int gwbp_neighbor_similarity_typed(int64_t n, int32_t D, int32_t k, const int32_t *idx, const void *features,
                                            int32_t field_type, int64_t ldf, float *sim, int32_t *live, void *stream);
GWBP_API int gwbp_edge_union(int64_t n, int32_t k, const int32_t *idx, const float *sim, const int32_t *live, const float *dist,
                             const int32_t *group, float sim_min, float max_dist, int32_t *count, int32_t *parent, int32_t *status,
                             void *stream);

/* ---- Point samples: what a finished field says at an arbitrary 3-D point, by the Gaussians' own shape (scale, rotation, opacity),
 * on the grid of the spatial search above ---------------------------------------------------------------------------------------------
 * means[n, 3], quats[n, 4] (wxyz, not normalised), scales[n, 3] (after exp), opacities[n] (after sigmoid): as for the projection, fp32,
 * read in place at row strides ldm >= 3, ldq >= 4, lds >= 3.  live[n] (optional, may be NULL: every Gaussian): uint8.  The contract:
 *   a Gaussian is LIVE when its mean is finite; its quaternion is finite with 0 < n2 < +inf, n2 = fmaf(q3, q3, fmaf(q2, q2, fmaf(q1,
 *     q1, q0 * q0))); its scales are finite and > 0; its opacity is finite and > 0; live[i] != 0;
 *   PACK, fp32, every operation written out and rounded once: inv = 1 / sqrtf(n2) (a correctly rounded sqrt and divide);
 *     (w, x, y, z) = (q0 inv, q1 inv, q2 inv, q3 inv); x2 = x x, y2 = y y, z2 = z z, xy = x y, xz = x z, yz = y z, wx = w x, wy = w y,
 *     wz = w z;  R (gsplat's quat_to_rotmat) = [1 - 2 (y2 + z2), 2 (xy - wz), 2 (xz + wy); 2 (xy + wz), 1 - 2 (x2 + z2), 2 (yz - wx);
 *     2 (xz - wy), 2 (yz + wx), 1 - 2 (x2 + y2)];  M[a][b] = R[b][a] / s[a], one correctly rounded divide each;  o = the opacity.
 *     A dead Gaussian has M = 0 and o = 0.  Rotate-then-divide on purpose: a precomputed inverse covariance loses (s_max / s_min)^2
 *     eps in sigma on needle-shaped Gaussians, this form about (|d| / s_min) eps |u|.  (q, -q and 2 q give the same bits.)
 *     The record: GWBP_SAMPLE_PACK = 12 floats, (M00 M01 M02 o) (M10 M11 M12 0) (M20 M21 M22 0);
 *   WEIGHT of Gaussian i at x: d = x - mean, each component in fp32; u_a = fmaf(M[a][2], d_z, fmaf(M[a][1], d_y, M[a][0] * d_x));
 *     m2 = fmaf(u_2, u_2, fmaf(u_1, u_1, u_0 * u_0)); sigma = 0.5f * m2; w = o * exp_neg(-sigma), exp_neg the blend's deterministic
 *     exponential (ln 2 range reduction, degree-7 Horner polynomial, no transcendental unit).  The weight is KEPT when sigma <= 80
 *     and w >= alpha_min, else it is 0.  alpha_min = 1/255 (0x1.010102p-8f) makes the rule "a Gaussian counts at a point exactly
 *     where the rasteriser would let it count at a pixel"; alpha_min in [GWBP_SAMPLE_MIN_ALPHA, 1], so that no subnormal is kept;
 *   the CANDIDATES of a query are the Gaussians with a finite mean whose centre has d2 <= r2, d2 gwbp_spatial_knn's expression, r2
 *     the caller's fp32 radius * radius as for gwbp_radius_count (a dead candidate has weight 0 and is never kept);
 *   the RESULT of a query: the k candidates of largest kept weight, ordered by (weight descending, index ascending): idx[q, k]
 *     (int32, original indices, tail -1), w[q, k] (fp32, tail 0), and n_contrib[q] (int32) = the number of candidates with a kept
 *     weight; n_contrib > k says the list was truncated.  A non-finite query gets the empty result.
 * The result is a pure function of the inputs: it does not depend on the grid, the launch or the order of the walk, and two runs give
 * the same bits.  Nothing is summed across candidates in the walk, which is why it returns a count and not a mass.
 *   gwbp_gaussian_pack     pack[p] (float [n, GWBP_SAMPLE_PACK], 16-B aligned) = the record of Gaussian perm[p]: the grid's SORTED
 *                          order (perm: the permutation gwbp_spatial_build was given), so that a walk position indexes it.
 *   gwbp_point_gaussians   the result above for the query rows queries[g * ldq + 0..2], g < q.  sorted / cell_start / the grid: what
 *                          gwbp_spatial_build made of the means.  order[q]: as for gwbp_spatial_knn.  visited (optional): int32 [q],
 *                          the number of Gaussians whose distance the query's lane computed.  Lane-private lists: no atomics.
 *   gwbp_neighbor_blend    over a list (idx[q, k], w[q, k]) and features[m, D] (row i at features + i * ldf): an entry with an index
 *                          outside [0, m) or with w == 0 is SKIPPED and its row is not read (a NaN row behind a zero weight does
 *                          not leak).  W = the chain acc = w_j + acc from +0 over the entries left, in list order; out[g * ldo + c]
 *                          = (the chain acc = fmaf(w_j, features[idx_j, c], acc) from +0, same order) / W, one correctly rounded
 *                          divide; wsum[g] = W.  A row with no entry left is zero and its wsum is 0.  Rows whose addresses and
 *                          strides are 16-B aligned move with 16-B loads and stores, with the same bits.  No atomics.
 *   gwbp_weighted_vote     over a list and labels[m] (int32): an entry takes part when it is not skipped (as above) and its label c
 *                          = labels[idx_j] is in [0, num_classes).  S[c] = the chain acc = w_j + acc from +0 over the entries of
 *                          class c, in list order; T = the same chain over all entries that take part.  out_label[g] = the class of
 *                          largest S, ties to the smallest class, -1 when nothing took part; out_share[g] = S[best] / T (0 then).
 * 1 <= n, m < 2^31; 0 <= q < 2^31; 1 <= k <= GWBP_SAMPLE_MAX_K; D >= 1; r2 >= 0 (+inf allowed); the grid as for gwbp_spatial_knn.
 * GWBP_EINVAL before any HIP call: a size, k, D, num_classes, r2, alpha_min, grid dimension, cell size or stride outside these, a
 * null required pointer, a misaligned pointer, an output array that is an input array or another output. */
#define GWBP_SAMPLE_PACK 12
#define GWBP_SAMPLE_MAX_K 32
#define GWBP_SAMPLE_MIN_ALPHA 1e-30f
GWBP_API int gwbp_gaussian_pack(int64_t n, const float *means, int64_t ldm, const float *quats, int64_t ldq, const float *scales,
                                int64_t lds, const float *opacities, const uint8_t *live, const int64_t *perm, float *pack,
                                void *stream);
GWBP_API int gwbp_point_gaussians(int64_t n, const float *sorted, const int32_t *cell_start, float lo_x, float lo_y, float lo_z,
                                  float cell_size, int32_t nx, int32_t ny, int32_t nz, const float *pack, float r2, float alpha_min,
                                  int64_t q, const float *queries, int64_t ldq, const int64_t *order, int32_t k, int32_t *idx, float *w,
                                  int32_t *n_contrib, int32_t *visited, void *stream);
GWBP_API int gwbp_neighbor_blend(int64_t q, int64_t m, int32_t D, int32_t k, const int32_t *idx, const float *w, const float *features,
                                 int64_t ldf, float *out, int64_t ldo, float *wsum, void *stream);

/* gwbp_neighbor_blend with a typed field `features`: `field_type` (GWBP_MAP_F32 / _F16 / _BF16) is the element type of that one operand and its row stride counts
 * ELEMENTS.  An unknown field_type is GWBP_EINVAL, checked before anything else; a field pointer that is not aligned to its element
 * (4 B, 2 B) is GWBP_EINVAL before any HIP call, as are the untyped function's own invalid cases.  GWBP_MAP_F32 does exactly what
 * the untyped function does (which is a call of this one).  A half field is widened to fp32 as it is loaded or staged -- exact --
 * so every result has the BITS the untyped function gives on the fp32 copy of the field, and no such copy is made.  Half rows whose
 * address is 8-B aligned and whose stride is a multiple of 4 elements move with one 8-B load per four channels, others element by
 * element, with the same bits. The weights w, out and wsum stay fp32. */
GWBP_API int gwbp_neighbor_blend_typed(int64_t q, int64_t m, int32_t D, int32_t k, const int32_t *idx, const float *w,
                                       const void *features, int32_t field_type, int64_t ldf, float *out, int64_t ldo, float *wsum,
                                       void *stream);
/* gwbp_neighbor_blend_typed with a typed OUTPUT, as gwbp_neighbor_mean_out_typed: out_type is the element type of out, ldo counts its
 * elements, a half out is the fp32 quotient rounded once to nearest even and must not be one of the inputs; wsum stays fp32.
 * gwbp_neighbor_blend_typed is a call of this function with GWBP_MAP_F32. */
GWBP_API int gwbp_neighbor_blend_out_typed(int64_t q, int64_t m, int32_t D, int32_t k, const int32_t *idx, const float *w,
                                           const void *features, int32_t field_type, int64_t ldf, void *out, int32_t out_type,
                                           int64_t ldo, float *wsum, void *stream);
GWBP_API int gwbp_weighted_vote(int64_t q, int64_t m, int32_t k, const int32_t *idx, const float *w, const int32_t *labels,
                                int32_t num_classes, int32_t *out_label, float *out_share, void *stream);

/* ---- PCA of a finished field (the reference's visualize_pca.py: sklearn PCA(3) on the host copy of the [N, D] field) -------------
 * The [N, D] passes of the fit and of the transform; the D x D eigen-decomposition between them is the caller's (float64 eigh of
 * gram / (N - 1); sklearn's covariance_eigh solver does the same).  X[g * ldx + 0..D-1], g < N, is read in place, fp32, any row
 * stride ldx >= D (in floats); rows whose addresses and stride are 16-B aligned are read with 16-B loads, others element by element,
 * with bit-equal results.  No [N, D] intermediate is made: x - mean is one fp32 subtraction on the way into LDS.  No atomics: every
 * output is bit-reproducible run to run.  2 <= N, 1 <= D <= GWBP_PCA_MAX_D.
 * GWBP_EINVAL before any HIP call: sizes out of range, a stride below D, a null or (X: 4-B, gram / workspace: 8-B) misaligned
 * pointer; GWBP_EWORKSPACE: a workspace below gwbp_pca_workspace_size. */
#define GWBP_PCA_MAX_D 2048
#define GWBP_PCA_MAX_K 16
#define GWBP_PCA_PROJECT_ROWS 128 /* rows of X per workgroup of gwbp_pca_project = per (min, max) pair of its partials */

/* Bytes of device workspace gwbp_column_means and gwbp_centered_gram need for an [N, D] field: the per-slice partial sums,
 * max(mean slices x D x 8, Gram slices x D x D x 4); the Gram's slices are min(512 / tiles, N / 32) with tiles = the 128 x 128
 * tiles of the upper triangle, so the figure never exceeds 64 MiB and never grows with N.  The workspace carries nothing between
 * calls. */
GWBP_API int gwbp_pca_workspace_size(int64_t N, int32_t D, size_t *bytes);

/* mean_out[c] = (1 / N) sum_g X[g, c]: float64 column sums per fixed row slice (ascending rows), the slices added in ascending
 * order in float64, one rounding to fp32. */
GWBP_API int gwbp_column_means(int64_t N, int32_t D, const float *X, int64_t ldx, float *mean_out, void *workspace,
                               size_t workspace_bytes, void *stream);

/* gwbp_column_means with a typed field X: `field_type` (GWBP_MAP_F32 / _F16 / _BF16) is the element type of that one operand and its row stride counts
 * ELEMENTS.  An unknown field_type is GWBP_EINVAL, checked before anything else; a field pointer that is not aligned to its element
 * (4 B, 2 B) is GWBP_EINVAL before any HIP call, as are the untyped function's own invalid cases.  GWBP_MAP_F32 does exactly what
 * the untyped function does (which is a call of this one).  A half field is widened to fp32 as it is loaded or staged -- exact --
 * so every result has the BITS the untyped function gives on the fp32 copy of the field, and no such copy is made.  Half rows whose
 * address is 8-B aligned and whose stride is a multiple of 4 elements move with one 8-B load per four channels, others element by
 * element, with the same bits. mean_out stays fp32, the workspace is the untyped function's. */
GWBP_API int gwbp_column_means_typed(int64_t N, int32_t D, const void *X, int32_t field_type, int64_t ldx, float *mean_out,
                                     void *workspace, size_t workspace_bytes, void *stream);

/* gram_out[a * D + b] (float64, dense [D, D], symmetric) = sum_g (X[g, a] - mean[a]) (X[g, b] - mean[b]).  The rows are cut into
 * slices that depend on (N, D) alone; within a slice every entry of the upper triangle is one chain of fp32 fused multiply-adds
 * over the rows (the fp32 matrix cores; no reduced-precision operand); the slices are added in ascending order in float64 and
 * the lower triangle is the mirror image.  A non-finite X entry makes the entries of its column non-finite. */
GWBP_API int gwbp_centered_gram(int64_t N, int32_t D, const float *X, int64_t ldx, const float *mean, double *gram_out,
                                void *workspace, size_t workspace_bytes, void *stream);

/* gwbp_centered_gram with a typed field X: `field_type` (GWBP_MAP_F32 / _F16 / _BF16) is the element type of that one operand and its row stride counts
 * ELEMENTS.  An unknown field_type is GWBP_EINVAL, checked before anything else; a field pointer that is not aligned to its element
 * (4 B, 2 B) is GWBP_EINVAL before any HIP call, as are the untyped function's own invalid cases.  GWBP_MAP_F32 does exactly what
 * the untyped function does (which is a call of this one).  A half field is widened to fp32 as it is loaded or staged -- exact --
 * so every result has the BITS the untyped function gives on the fp32 copy of the field, and no such copy is made.  Half rows whose
 * address is 8-B aligned and whose stride is a multiple of 4 elements move with one 8-B load per four channels, others element by
 * element, with the same bits. mean stays fp32, gram_out float64, the workspace is the untyped function's. */
GWBP_API int gwbp_centered_gram_typed(int64_t N, int32_t D, const void *X, int32_t field_type, int64_t ldx, const float *mean,
                                      double *gram_out, void *workspace, size_t workspace_bytes, void *stream);

/* Y[g * k + j] = sum_c (X[g, c] - mean[c]) components[j * D + c], j < k <= GWBP_PCA_MAX_K: one pass over X, one chain of fp32
 * fused multiply-adds per entry in an order that depends only on D.  minmax_partials[2 * w], [2 * w + 1], w < ceil(N /
 * GWBP_PCA_PROJECT_ROWS): the smallest and the largest Y entry of rows w * GWBP_PCA_PROJECT_ROWS ...; min and max are exact, so
 * the smallest / largest of them is Y's (NaN entries are skipped).  N >= 1 here. */
GWBP_API int gwbp_pca_project(int64_t N, int32_t D, int32_t k, const float *X, int64_t ldx, const float *mean,
                              const float *components, float *Y, float *minmax_partials, void *stream);

/* gwbp_pca_project with a typed field X: `field_type` (GWBP_MAP_F32 / _F16 / _BF16) is the element type of that one operand and its row stride counts
 * ELEMENTS.  An unknown field_type is GWBP_EINVAL, checked before anything else; a field pointer that is not aligned to its element
 * (4 B, 2 B) is GWBP_EINVAL before any HIP call, as are the untyped function's own invalid cases.  GWBP_MAP_F32 does exactly what
 * the untyped function does (which is a call of this one).  A half field is widened to fp32 as it is loaded or staged -- exact --
 * so every result has the BITS the untyped function gives on the fp32 copy of the field, and no such copy is made.  Half rows whose
 * address is 8-B aligned and whose stride is a multiple of 4 elements move with one 8-B load per four channels, others element by
 * element, with the same bits. mean, components, Y and minmax_partials stay fp32. */
GWBP_API int gwbp_pca_project_typed(int64_t N, int32_t D, int32_t k, const void *X, int32_t field_type, int64_t ldx, const float *mean,
                                    const float *components, float *Y, float *minmax_partials, void *stream);

/* colors[e] = (Y[e] - lo) / (hi - lo), e < n, with lo = lo_hi[0], hi = lo_hi[1] read from DEVICE memory (one pair for every
 * channel: visualize_pca.py takes np.min / np.max over all three); hi == lo gives 0.5 everywhere.  colors may alias Y. */
GWBP_API int gwbp_pca_colors(int64_t n, const float *Y, const float *lo_hi, float *colors, void *stream);

/* ---- Clustering a finished field: the two [N, D] passes of a k-means (Lloyd) step (cluster.hip) -----------------------------------
 * gwbp_kmeans_assign: for every row X[g * ldx + 0..D-1], g < N, against the K centroid rows C[j * ldc + 0..D-1]:
 *   score(g, j) = <X[g, :], C[j, :]> + b[j],   label[g] = argmax_j score(g, j) (int32 [N]),   best[g] = that score (fp32 [N]).
 * The inner product is gwbp_knn_search's score bit for bit: one chain of fp32 fused multiply-adds over the D index in an order that
 * depends only on D (the fp32 matrix cores; no reduced-precision operand).  b (fp32 [K], may be NULL): with NULL the score is the
 * chain itself -- the cosine / inner-product metric, and label / best equal column 0 of gwbp_knn_search(..., k = 1) bit for bit on
 * rows that have a score that is a number; otherwise ONE fp32 addition of b[j] follows the finished chain.  b[j] = -|c_j|^2 / 2
 * (computed by the caller in float64, rounded once) makes the argmax the Euclidean nearest centroid.  Ties go to the lowest index,
 * -0 counts as +0 (and is returned as +0); a NaN score orders after every number and is never chosen: a row whose scores are all
 * NaN gets label -1 and best NaN.  No score reaches global memory, there is no top-k list and no workspace.  X and C are read in
 * place at any row stride >= D (in floats); rows whose addresses and strides are 16-B aligned are read with 16-B loads, others
 * element by element (same results).  1 <= K <= GWBP_CLUSTER_MAX_K, D >= 1.
 * GWBP_EINVAL before any HIP call: N < 0, K < 1 or K > GWBP_CLUSTER_MAX_K, D < 1, ldx < D, ldc < D, a null X (N > 0), C, label or
 * best (N > 0), a pointer that is not 4-B aligned. */
#define GWBP_CLUSTER_MAX_K (1 << 20)
#define GWBP_CLUSTER_RUN 256 /* members per run of gwbp_cluster_sums: part of its arithmetic contract */
GWBP_API int gwbp_kmeans_assign(int64_t N, int32_t K, int32_t D, const float *X, int64_t ldx, const float *C, int64_t ldc,
                                const float *b, int32_t *label, float *best, void *stream);

/* gwbp_kmeans_assign with a typed field X: `field_type` (GWBP_MAP_F32 / _F16 / _BF16) is the element type of that one operand and its row stride counts
 * ELEMENTS.  An unknown field_type is GWBP_EINVAL, checked before anything else; a field pointer that is not aligned to its element
 * (4 B, 2 B) is GWBP_EINVAL before any HIP call, as are the untyped function's own invalid cases.  GWBP_MAP_F32 does exactly what
 * the untyped function does (which is a call of this one).  A half field is widened to fp32 as it is loaded or staged -- exact --
 * so every result has the BITS the untyped function gives on the fp32 copy of the field, and no such copy is made.  Half rows whose
 * address is 8-B aligned and whose stride is a multiple of 4 elements move with one 8-B load per four channels, others element by
 * element, with the same bits. The centroids C, the bias b, label and best stay fp32 / int32. */
GWBP_API int gwbp_kmeans_assign_typed(int64_t N, int32_t K, int32_t D, const void *X, int32_t field_type, int64_t ldx, const float *C,
                                      int64_t ldc, const float *b, int32_t *label, float *best, void *stream);

/* Bytes of device workspace gwbp_cluster_sums needs: the per-run partial sums, (min(N, ceil(N / GWBP_CLUSTER_RUN) + K)) x (D + 1)
 * float64, plus K + 1 int64.  The workspace carries nothing between calls.  GWBP_EINVAL: N < 0, K or D out of range, null bytes. */
GWBP_API int gwbp_cluster_workspace_size(int64_t N, int32_t D, int32_t K, size_t *bytes);

/* Per-cluster, optionally weighted, column sums of the rows of X (the k-means update; the class prototypes of a labelling):
 *   sums[k * D + c] = sum_{g: label[g] = k} w[g] X[g * ldx + c]  (float64, dense [K, D]),   wsum[k] = sum w[g]  (float64 [K]).
 * The caller groups the rows first: order[N] (int64) lists the rows by label ascending, row index ascending inside a label (a
 * STABLE sort of the labels), and start[K + 1] (int64) holds the first position of every label in it, start[K] the end of label
 * K - 1.  Rows before start[0] and from start[K] on -- labels outside [0, K) -- take no part.  w (fp32 [N], may be NULL: weights
 * of 1) is indexed by row.  Contract: every term w x is formed in float64 (exact); a cluster's member list is cut into runs of
 * GWBP_CLUSTER_RUN members; each (run, column) is summed in float64 in ascending member order; a cluster's runs are added in
 * ascending order; no atomics.  The result depends on (X, labels, w) alone: two runs, another stream, another alignment (16-B
 * loads where addresses allow, element loads otherwise) give the same bits.  A cluster without members gets a zero row and wsum 0.
 * Entries of order outside [0, N) are skipped and start values are clamped into [0, N]: no call reads outside X.
 * GWBP_EINVAL before any HIP call: N < 0, K < 1 or K > GWBP_CLUSTER_MAX_K, D < 1, ldx < D, a null X or order (N > 0), a null
 * start, sums, wsum or workspace, a pointer that is not aligned to its element (X, w: 4 B; the others: 8 B);
 * GWBP_EWORKSPACE: a workspace below gwbp_cluster_workspace_size. */
GWBP_API int gwbp_cluster_sums(int64_t N, int32_t D, int32_t K, const float *X, int64_t ldx, const float *w, const int64_t *order,
                               const int64_t *start, double *sums, double *wsum, void *workspace, size_t workspace_bytes,
                               void *stream);

/* gwbp_cluster_sums with a typed field X: `field_type` (GWBP_MAP_F32 / _F16 / _BF16) is the element type of that one operand and its row stride counts
 * ELEMENTS.  An unknown field_type is GWBP_EINVAL, checked before anything else; a field pointer that is not aligned to its element
 * (4 B, 2 B) is GWBP_EINVAL before any HIP call, as are the untyped function's own invalid cases.  GWBP_MAP_F32 does exactly what
 * the untyped function does (which is a call of this one).  A half field is widened to fp32 as it is loaded or staged -- exact --
 * so every result has the BITS the untyped function gives on the fp32 copy of the field, and no such copy is made.  Half rows whose
 * address is 8-B aligned and whose stride is a multiple of 4 elements move with one 8-B load per four channels, others element by
 * element, with the same bits. The weights w stay fp32, sums and wsum float64, the workspace is the untyped
 * function's. */
GWBP_API int gwbp_cluster_sums_typed(int64_t N, int32_t D, int32_t K, const void *X, int32_t field_type, int64_t ldx, const float *w,
                                     const int64_t *order, const int64_t *start, double *sums, double *wsum, void *workspace,
                                     size_t workspace_bytes, void *stream);

/* ---- questions asked of a finished field (the reference's segment.py, segment_compressed.py, click_and_segment.py) ---------------
 * Scores of every row of X[g * ldx + 0..D-1], g < N, against P prompt vectors prompts[j * D + 0..D-1] (dense), and the 3-D mask of
 * get_mask3d_lseg, in ONE pass over X; no workspace, no view.
 *   s[g, j]  = X[g] . prompts[j] / max(|X[g]|_2, 1e-12)  with normalize != 0 (F.normalize's rule: a zero row scores 0), the bare
 *              dot product otherwise (click_and_segment.py's form)
 *   mask[g]  = max_{j < n_pos} s[g, j] > max_{j >= n_pos} s[g, j], ANDed with s[g, 0] > *threshold_host when that pointer is given
 *              (read on the host at the call).  n_pos == P: no negatives, the mask is the threshold test alone and the threshold
 *              is required.  A NaN score loses every comparison (the maxima propagate NaN as torch.max does).
 * mask (uint8 [N], 0 / 1) and scores (fp32 [N, P] dense) may each be NULL, not both.  1 <= P <= GWBP_QUERY_MAX_P (the channel limit
 * of gwbp_render_pixels, which renders the scores), 1 <= n_pos <= P, 1 <= D <= GWBP_PCA_MAX_D, ldx >= D, N >= 0.
 * Arithmetic: every dot product and the row's sum of squares is one chain of fp32 fused multiply-adds over the channel index in
 * an order that depends only on D (the fp32 matrix cores; no reduced-precision operand); one correctly rounded sqrt and divide.
 * Results do not depend on the row's position, on N, P or the launch; rows whose address and stride are 16-B aligned are read with
 * 16-B loads, others element by element, with bit-equal results; padding beyond D is never read; no atomics.
 * GWBP_EINVAL before any HIP call: sizes out of range, a stride below D, a null or (4-B) misaligned X or prompts, both outputs
 * null, no negatives and no threshold. */
#define GWBP_QUERY_MAX_P 32
GWBP_API int gwbp_prompt_scores(int64_t N, int32_t D, int32_t P, int32_t n_pos, const float *X, int64_t ldx, const float *prompts,
                                int32_t normalize, const float *threshold_host, uint8_t *mask, float *scores, void *stream);

/* gwbp_prompt_scores with a typed field X: `field_type` (GWBP_MAP_F32 / _F16 / _BF16) is the element type of that one operand and its row stride counts
 * ELEMENTS.  An unknown field_type is GWBP_EINVAL, checked before anything else; a field pointer that is not aligned to its element
 * (4 B, 2 B) is GWBP_EINVAL before any HIP call, as are the untyped function's own invalid cases.  GWBP_MAP_F32 does exactly what
 * the untyped function does (which is a call of this one).  A half field is widened to fp32 as it is loaded or staged -- exact --
 * so every result has the BITS the untyped function gives on the fp32 copy of the field, and no such copy is made.  Half rows whose
 * address is 8-B aligned and whose stride is a multiple of 4 elements move with one 8-B load per four channels, others element by
 * element, with the same bits. The prompts, the threshold, mask and scores stay fp32 / uint8. */
GWBP_API int gwbp_prompt_scores_typed(int64_t N, int32_t D, int32_t P, int32_t n_pos, const void *X, int32_t field_type, int64_t ldx,
                                      const float *prompts, int32_t normalize, const float *threshold_host, uint8_t *mask,
                                      float *scores, void *stream);

/* The field rendered at M pixels only (click_and_segment.py:241-254 renders all [H, W, D + 1] values to read one pixel's): needs
 * gwbp_project (or gwbp_project_camera) + gwbp_bin_sort of the view in the workspace, like gwbp_render_pixels; no weight store.
 *   out[m, :] = sum_g w_g(p_m) X[g, :]   depth[m] = sum_g w_g(p_m) z_g (z: the projection's camera depth; gsplat's accumulated "D"
 *   channel, not the expected depth)   alpha[m] = 1 - T          p_m = (xy[2 m], xy[2 m + 1]) = (x, y), int32 on the DEVICE
 * X[g * ldx + 0..D-1] has a row for every Gaussian of the caps.  out is dense [M, D]; depth and alpha ([M]) may be NULL.  A pixel
 * outside the image gives a zero row, depth 0 and alpha 0.  The weights are the blend's bit for bit, and every channel is summed
 * front to back with fmaf(w, x, acc): the result equals that pixel of gwbp_render / gwbp_render_pixels of the same table.
 * 1 <= M <= GWBP_PROBE_MAX_PIXELS, 1 <= D <= GWBP_PCA_MAX_D, ldx >= D.
 * GWBP_EINVAL before the workspace is looked at: sizes out of range, a stride below D, a null or (4-B) misaligned xy, X or out. */
#define GWBP_PROBE_MAX_PIXELS 4096
GWBP_API int gwbp_probe_pixels(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                               int32_t M, const int32_t *xy, const float *X, int64_t ldx, int32_t D, float *out, float *depth,
                               float *alpha, void *stream);

/* gwbp_probe_pixels with a typed table X: `field_type` (GWBP_MAP_*) is its element type and ldx counts ELEMENTS.  An unknown
 * field_type is GWBP_EINVAL, checked before anything else; an X that is not aligned to its element is GWBP_EINVAL with the probe's own
 * invalid cases, before the workspace is looked at.  A half row is widened -- exact -- as it is loaded (8-B loads of four elements
 * where X is 8-B aligned and ldx a multiple of 4, 2-B loads otherwise): out, depth and alpha have the bits of gwbp_probe_pixels on the
 * fp32 copy of X, and no such copy is made.  gwbp_probe_pixels is a call of this function with GWBP_MAP_F32. */
GWBP_API int gwbp_probe_pixels_typed(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                                     int32_t M, const int32_t *xy, const void *X, int32_t field_type, int64_t ldx, int32_t D, float *out,
                                     float *depth, float *alpha, void *stream);

/* The Gaussians a pixel is made of -- the 2-D counterpart of gwbp_point_gaussians: needs gwbp_project (or gwbp_project_camera) +
 * gwbp_bin_sort of the view in the workspace, like gwbp_render_pixels; no weight store.  It reads the workspace and writes nothing
 * into it.  xy == NULL: every pixel of the view, P = height * width, row-major, M ignored.  xy != NULL: the P = M pixels p_m = (xy[2 m],
 * xy[2 m + 1]) = (x, y), int32 on the DEVICE, 1 <= M <= GWBP_PROBE_MAX_PIXELS; a pixel outside the image gives an empty list,
 * n_contrib 0, alpha 0 and median -1.  Both forms give the same bits at the same pixel.  With w_g(p) = alpha T, the blend's bits:
 *   ids int32 [P, k], weights float [P, k]: the k contributing records of largest weight, by weight descending, equal weights by
 *             Gaussian id ascending; empty slots hold id -1 and weight 0.  1 <= k <= GWBP_PIXEL_TOPK_MAX.  With k >= n_contrib[p] the
 *             list is the complete row p of the view's weight matrix.
 *   n_contrib int32 [P]: the number of contributing records; n_contrib[p] > k means the list was cut.
 *   alpha float [P]: 1 - T, the bits of gwbp_render_pixels' alphas.
 *   median_id int32 [P], median_depth float [P]: the first contributing record, in list (depth) order, after which T <= 0.5, and its
 *             camera depth (the projection's: the z gwbp_probe_pixels' depth accumulates); -1 and 0 where T stays above one half.
 * ids and weights are required; the other four may be NULL, which costs no store.
 * GWBP_EINVAL before the workspace is looked at: k out of range, M out of range (with xy), a null or (4-B) misaligned ids or weights,
 * a misaligned xy or optional output. */
#define GWBP_PIXEL_TOPK_MAX 16
GWBP_API int gwbp_pixel_gaussians(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host, int32_t k,
                                  int32_t M, const int32_t *xy, int32_t *ids, float *weights, int32_t *n_contrib, float *alpha,
                                  int32_t *median_id, float *median_depth, void *stream);

/* ---- per-Gaussian labels rendered to 2-D class maps and scored (the reference's evaluate_results and render_affordance,
 * affordance_transfer/demo_affordance_transfer.py:1445-1611, 1399-1439) ------------------------------------------------------------
 * One blend pass over a projected and sorted view (gwbp_project or gwbp_project_camera + gwbp_bin_sort, like gwbp_render_pixels; no
 * weight store) with ONE int32 per Gaussian as its payload: labels[g], g < caps->n_gaussians.  A label outside [0, num_classes)
 * contributes to alpha and to no class.  Every output may be NULL (not all of them); a NULL output costs no store.
 *   maps   float [H, W, num_classes]: maps[p, k] = sum of w_g(p) over the Gaussians of label k, front to back.  Equal bit for bit
 *          to the gwbp_render_pixels / gwbp_render of the one-hot [N, num_classes] table, which nobody has to build.
 *   alphas float [H, W]: as gwbp_render_pixels.
 *   argmax int32 [H, W]: the class of the largest sum, the lowest index among equals; -1 where no class has a sum above 0 or the
 *          largest sum lies below min_opacity.  argmax_sums float [H, W]: that largest sum (0 where nothing contributed); it is
 *          the carry between the chunks of 64 classes a wide table is rendered in, so argmax needs it from num_classes > 64 on.
 *   counts uint64 [num_classes, 3]: {intersection, predicted, ground truth} pixel counts of every class against gt (int32 [H, W],
 *          dense), ADDED to what is there:
 *            predicted(p, k)    <=>  fl32(min(max(maps[p, k], 0), 1) * 255.0f) >= cut + 1   (the reference's
 *                                    torch_to_cv(render) > cut: clamp, one fp32 multiply, truncation to uint8; cut = 64 there)
 *            ground truth(p, k) <=>  gt[p] == k   (a value outside [0, num_classes) matches no class)
 *          Integer atomics only: the counts do not depend on the order of the additions.  gt and counts come together.
 * num_classes > 64 costs one blend pass per 64 classes (class sums are independent: the result is that of one pass).
 * GWBP_EINVAL before the workspace is looked at: num_classes outside [1, GWBP_RENDER_LABELS_MAX_CLASSES], null or misaligned
 * labels, every output null, a misaligned output (counts: 8 B, others 4 B), argmax of more than 64 classes without argmax_sums,
 * gt without counts or counts without gt, cut outside [0, 255]. */
#define GWBP_RENDER_LABELS_MAX_CLASSES 65536
GWBP_API int gwbp_render_labels(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                                const int32_t *labels, int32_t num_classes, float *maps, float *alphas, int32_t *argmax,
                                float *argmax_sums, float min_opacity, const int32_t *gt, int32_t cut, uint64_t *counts,
                                void *stream);

/* ---- a finished field scored against the 2-D map of a view it was lifted from ------------------------------------------------------
 * Needs the view's weight store in the workspace, exactly as gwbp_render does (gwbp_project or gwbp_project_camera + gwbp_bin_sort +
 * a storing blend).  With r(p) = sum_g w_g(p) features[g * ldf + 0..D-1] -- gwbp_render's values bit for bit: the same front-to-back
 * fmaf chain per pixel and channel -- and m(p, :) the map row of pixel p, the kernel forms per pixel, in fp32,
 *     dot = sum_c r m     rr = sum_c r r     mm = sum_c m m     l1 = sum_c |r - m|     l2 = sum_c (r - m)^2
 * and cosine = dot / sqrt(rr mm) (float64 arithmetic on the fp32 sums, one rounding to fp32; NaN where rr mm == 0).  The [H, W, D]
 * render is never made.
 *   map     element type map_type (GWBP_MAP_F32 / F16 / BF16, read natively with the value of a conversion to fp32), unit channel
 *           stride, pixel (y, x) at map + y * ms_y + x * ms_x (strides in elements, >= 0).  Full resolution [H, W, D] with ymap =
 *           xmap = NULL; or a low-resolution [lr_h, lr_w, D] map with ymap int32 [H] / xmap int32 [W], the row / column of every
 *           output row / column (F.interpolate(mode="nearest")'s index maps; clamped into the map by the kernel).
 *   planes  float [6][H][W] or NULL: dot, rr, mm, l1, l2, cosine.  NULL costs no store.
 *   table   double [8], overwritten: sum cosine, sum l1, sum l2, sum mm, n_valid, n_bad, n_pixels (= H W), D.
 * A pixel whose map row holds a non-finite element is BAD: NaN in all six planes, counted in n_bad.  A pixel is VALID when it is not
 * bad, its five sums are finite, rr > 0 and mm > 0; the four sums of the table run over the valid pixels only.  Pixels of a partial
 * edge tile outside the image are neither read nor written.
 * Order of additions (depends on D alone -- not on alignment, the map's type or shape): per block of 256 channels a lane's four
 * channels in ascending order, the 64 lanes by a fixed tree, the blocks in ascending order; the table in float64: a tile row's 16
 * pixels by a fixed butterfly, the rows in a fixed order.  No atomics: two calls give the same bits, and the table does not depend
 * on whether planes are asked for.  Rows whose addresses and strides allow 16-B (field) and four-element (map) loads are read so,
 * others element by element, with bit-equal results.
 * The rows' partial sums use the workspace's carry slices (the 256-channel scatter kernel's): like every call on a workspace, it
 * must not run beside another call on the same workspace.  Views of at most GWBP_FIELD_COMPARE_MAX_TILES 16 x 16 tiles.
 * GWBP_EINVAL (after the caps, the workspace and the view, before any HIP call): an unknown map type, D outside [1, GWBP_PCA_MAX_D],
 * ldf < D, null or misaligned features (a scene of 0 Gaussians may pass NULL), map, index maps, planes (4 B) or table (8 B), negative
 * strides, one index map without the other, index maps without lr_h, lr_w >= 1, more tiles than the limit. */
#define GWBP_FIELD_COMPARE_MAX_TILES 262144
GWBP_API int gwbp_field_compare(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                                const float *features, int64_t ldf, int32_t D, const void *map, int32_t map_type, int64_t ms_y,
                                int64_t ms_x, int32_t lr_h, int32_t lr_w, const int32_t *ymap, const int32_t *xmap, float *planes,
                                double *table, void *stream);

/* gwbp_field_compare with a typed FIELD: `field_type` (GWBP_MAP_*) is the element type of features and ldf counts ELEMENTS; the map
 * keeps its own map_type.  An unknown field_type is GWBP_EINVAL, checked before anything else; features not aligned to its element is
 * GWBP_EINVAL with the function's other invalid cases.  A half field is read as stored -- the walk keeps the bits its loads landed and
 * widens them, exact, where they are multiplied; 8-B loads of four elements where rows allow them, 2-B loads otherwise -- so the
 * planes and the table have the bits of gwbp_field_compare on the fp32 copy of the field, whatever the map's type, and no such copy is
 * made.  The reduction order is the one documented above.  gwbp_field_compare is a call of this function with GWBP_MAP_F32. */
GWBP_API int gwbp_field_compare_typed(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                                      const void *features, int32_t field_type, int64_t ldf, int32_t D, const void *map,
                                      int32_t map_type, int64_t ms_y, int64_t ms_x, int32_t lr_h, int32_t lr_w, const int32_t *ymap,
                                      const int32_t *xmap, float *planes, double *table, void *stream);

/* ---- a latent field and its decoder: decode, compare and the gradients back through the decoder, in one call ----------------------
 * Between the render of a [N, d] latent table and the scatter of its gradient (gwbp_render, gwbp_scatter).  Takes no workspace of a
 * view: R [P, d] are the rendered rows of the P = height * width pixels (row-major, row stride ldr), C [d, D] the decoder (row
 * stride ldc), map the view's [height, width, D] map (GWBP_MAP_*, unit channel stride, pixel (y, x) at map + y * ms_y + x * ms_x,
 * strides in elements, >= 0), pixel_weights an optional per-pixel weight c_p (NULL: 1).  With w_p = scale * c_p (one rounding),
 *     y[p, j] = sum_k R[p, k] C[k, j]      e = y - map[p, j]
 *     g = w_p sign(e), sign(0) = 0  (GWBP_LOSS_L1)    |    g = w_p (e + e)  (GWBP_LOSS_L2)
 *     table[0] = loss = sum w_p |e|  |  sum w_p e^2                                      (float64)
 *     GR[p, :] = sum_j g[p, j] C[:, j]     float [P, d], row stride ldg; GR may be R itself
 *     GC[k, j] = sum_p R[p, k] g[p, j]     float [d, D], row stride ldgc
 *     table    = loss, n_pixels (not bad), n_bad, P, d, D, 0, 0                          (double [8], overwritten)
 * No [P, D] array is made: two kernels derive g by the same fused-multiply-add chain.  A pixel whose map row holds a non-finite
 * element is BAD: it adds nothing to the loss, GR or GC, its GR row is zero, and it counts in n_bad.
 * Arithmetic: every product sum is one chain of fp32 fused multiply-adds (v_mfma_f32_16x16x4_f32) from +0 in an order fixed by
 * (d, D) and the slice plan, which depends on P alone: 64-pixel blocks, ceil(blocks / GWBP_DECODE_MAX_SLICES) blocks per slice; GC
 * and the loss are the slices' partials added in ascending order in float64 (csrc/decode_loss.hip gives every order).  No atomics:
 * two calls give the same bits, and they do not depend on alignment, strides, the map's type beyond its values, or aliasing.
 * workspace: gwbp_decode_loss_workspace_size(d, D) bytes (the slices' partials: a function of d and D alone, never of P), 8-B
 * aligned, free again when the call's kernels have run.
 * GWBP_EUNSUPPORTED (before anything else but the pixel weights): d % 16 != 0 or d outside [16, 128], D % 16 != 0 or D outside
 * [16, GWBP_PCA_MAX_D], more than GWBP_DECODE_MAX_PIXELS pixels.  GWBP_EINVAL: negative height or width, an unknown map type or
 * loss kind, row strides below the row lengths, negative map strides, null or misaligned C, GC, table or workspace -- and R, map or
 * GR when P > 0 (4 B; the map to its element type; table and workspace 8 B).  GWBP_EWORKSPACE: a workspace below the size. */
#define GWBP_LOSS_L1 0
#define GWBP_LOSS_L2 1
#define GWBP_DECODE_MAX_SLICES 512
#define GWBP_DECODE_MAX_PIXELS (1 << 25)
GWBP_API int gwbp_decode_loss_workspace_size(int32_t d, int32_t D, size_t *bytes);
GWBP_API int gwbp_decode_loss(int32_t height, int32_t width, int32_t d, int32_t D, const float *R, int64_t ldr, const float *C,
                              int64_t ldc, const void *map, int32_t map_type, int64_t ms_y, int64_t ms_x,
                              const gwbp_pixel_weights *pixel_weights, int32_t loss_kind, float scale, float *GR, int64_t ldg,
                              float *GC, int64_t ldgc, double *table, void *workspace, size_t workspace_bytes, void *stream);

/* ---- the photometric loss of 3DGS training: (1 - lambda) L1 + lambda (1 - SSIM), its sums and its gradient, in one call -------------
 * x is the render, y the target: float32 [height, width, D], 1 <= D <= GWBP_IMAGE_LOSS_MAX_D, unit channel stride, pixel (r, c) at
 * x + (r * width + c) * xs (flat pixel rows; xs, ys >= D in elements, each tensor its own).  pixel_weights: an optional [height,
 * width] map w (NULL: 1).  Everything is per channel.  SSIM is the 11-tap, sigma 1.5 Gaussian-window form with C1 = 0.01^2,
 * C2 = 0.03^2 (data range 1); DESIGN.md 4 gives the arithmetic, csrc/ssim_math.h its expressions in their order.
 * padding GWBP_SSIM_VALID: the windows wholly inside the image, centres 5 <= r < height - 5, 5 <= c < width - 5 (needs height, width
 * >= 11); GWBP_SSIM_SAME: all height * width windows, zeros outside the image.
 *     table = sum w(q) ssim(q), sum w(p) |x - y|, sum w(p) (x - y)^2, Wv = sum over windows w(q), Wa = sum over pixels w(p),
 *             the number of windows, height * width, D                                       (double [8], overwritten)
 *     loss  = (1 - lambda) table[1] / (D Wa) + lambda (1 - table[0] / (D Wv))               (the caller's; a zero weight sum: 0)
 *     map   (NULL: not stored) float [H', W', D], the SSIM of every window and channel
 *     grad  (NULL: no backward) float [height, width, D] at pixel stride gs >= D: d loss / d x.  y receives no gradient.
 * Non-finite inputs are not masked: they propagate into the sums and the gradient.
 * One forward launch over tiles of GWBP_SSIM_TILE_Y x GWBP_SSIM_TILE_X pixels, one reduce launch (the tiles' float64 partials in
 * ascending tile order) and, with grad, one backward launch that reads Wv and Wa from the table on the device: no host read, no
 * atomics, two calls give the same bits, and a blur's chain does not depend on the tiling.
 * workspace: gwbp_image_loss_workspace_size(height, width, D, want_grad) = 40 * tiles + (want_grad ? 12 * height * width * D : 0)
 * bytes, tiles = ceil(height / GWBP_SSIM_TILE_Y) * ceil(width / GWBP_SSIM_TILE_X); 8-B aligned; free when the kernels have run.
 * GWBP_EINVAL: D outside [1, GWBP_IMAGE_LOSS_MAX_D], height or width < 1 (< 11 under GWBP_SSIM_VALID) or more than
 * GWBP_IMAGE_LOSS_MAX_PIXELS pixels, an unknown padding, pixel strides below D, null or misaligned x, y, table or workspace (4 B;
 * table and workspace 8 B), a misaligned map or grad.  GWBP_EWORKSPACE: a workspace below the size. */
#define GWBP_SSIM_VALID 0
#define GWBP_SSIM_SAME 1
#define GWBP_SSIM_TILE_Y 16
#define GWBP_SSIM_TILE_X 64
#define GWBP_IMAGE_LOSS_MAX_D 32
#define GWBP_IMAGE_LOSS_MAX_PIXELS (1 << 26)
GWBP_API int gwbp_image_loss_workspace_size(int32_t height, int32_t width, int32_t D, int32_t want_grad, size_t *bytes);
GWBP_API int gwbp_image_loss(int32_t height, int32_t width, int32_t D, const float *x, int64_t xs, const float *y, int64_t ys,
                             const gwbp_pixel_weights *pixel_weights, int32_t padding, float ssim_lambda, float *map, float *grad,
                             int64_t gs, double *table, void *workspace, size_t workspace_bytes, void *stream);

/* ---- densification: growing and pruning the set of Gaussians during training (gsplat's DefaultStrategy) --------------
 * Four calls that need no workspace of a view.  All arrays are dense unless a stride is named; float32 unless a type is named.  No
 * atomics: the same inputs give the same bits.  csrc/densify_math.h holds the expressions in their order.
 *
 * gwbp_densify_accumulate  (every training step)  v_means2d [n_cameras, n, 2]: d loss / d (2-D mean) in pixels, as
 *     rasterization(means2d_grad=True) leaves it in meta["means2d"].grad; radii int32 [n_cameras, n].  For each camera in order, where
 *     radii > 0:  grad2d[i] += sqrtf(a a + b b), a = gx sx, b = gy sy;  count[i] += 1.   (sx = W / 2 n_cameras, sy = H / 2 n_cameras)
 * gwbp_densify_plan  kind[i] (uint8, GWBP_DENSIFY_KIND_*) and offsets (int64 [n + 1]), the exclusive scan of the rows each Gaussian
 *     leaves behind (0, 1, 2, 2); offsets[n] is the size of the new set.  With m = the largest of scaling[i, 0..2] (logs; row stride
 *     lds), g = grad2d[i] / max(count[i], 1), low = opacity[i] < t_opa (logits), high = g > t_grad, small = m <= t_small:
 *         low -> pruned;  high and not small -> split, pruned if prune_big and m - log16 > t_big;
 *         else pruned if prune_big and m > t_big;  else clone if high, keep if not.
 *     Every comparison is in pre-activation space; one with a NaN is false.  workspace: gwbp_densify_plan_workspace_size(n) bytes, 8-B
 *     aligned, free when the kernels have run.  n = 0 writes offsets[0] = 0.
 * gwbp_densify_emit  every parent p writes its children at rows offsets[p] ..: parent (int32 [n_out]), child (uint8 [n_out]: 0 the
 *     original or first child, 1 the second) and the new means [n_out, 3], scaling [n_out, 3], rotation [n_out, 4], opacity [n_out].
 *     keep and clone copy the row's bits.  split, child k: mean + R(q / |q|) (exp(scaling) * noise[p, k, :]), scaling - log16, rotation
 *     and opacity copied; noise [n, 2, 3] is read on split rows only.  A row at or beyond n_out is not written.
 * gwbp_densify_gather  out[r, 0..w) = table[parent[r], 0..w) for r < n_out (row strides ldt, ldo >= w).  mode GWBP_DENSIFY_ZERO_NEW
 *     (optimiser moments): a row whose parent was split, or was cloned and child[r] != 0, is zeros instead; so is a row whose parent lies
 *     outside [0, n).  GWBP_DENSIFY_COPY reads neither child nor kind (they may be NULL).
 * GWBP_EINVAL before any HIP call: n outside [0, 2^31 - 1], n_cameras < 1, n_out outside [0, 2 n], w outside
 * [1, GWBP_DENSIFY_MAX_WIDTH], a row stride below its row, an unknown mode, a null or misaligned array (4 B; v_means2d, offsets and the
 * workspace 8 B) where n (n_out) > 0.  Whether n_out IS offsets[n] cannot be seen on the host: the kernels check every row index instead.
 * GWBP_EWORKSPACE: a workspace below the size. */
#define GWBP_DENSIFY_KIND_PRUNED 0
#define GWBP_DENSIFY_KIND_KEEP 1
#define GWBP_DENSIFY_KIND_CLONE 2
#define GWBP_DENSIFY_KIND_SPLIT 3
#define GWBP_DENSIFY_COPY 0
#define GWBP_DENSIFY_ZERO_NEW 1
#define GWBP_DENSIFY_BLOCK 256
#define GWBP_DENSIFY_GATHER_MAX_ROWS 1024
#define GWBP_DENSIFY_MAX_WIDTH 65536
GWBP_API int gwbp_densify_accumulate(int64_t n, int32_t n_cameras, const float *v_means2d, const int32_t *radii, float sx, float sy,
                                     float *grad2d, float *count, void *stream);
GWBP_API int gwbp_densify_plan_workspace_size(int64_t n, size_t *bytes);
GWBP_API int gwbp_densify_plan(int64_t n, const float *grad2d, const float *count, const float *scaling, int64_t lds,
                               const float *opacity, float t_grad, float t_small, float t_big, float t_opa, float log16,
                               int32_t prune_big, uint8_t *kind, int64_t *offsets, void *workspace, size_t workspace_bytes,
                               void *stream);
GWBP_API int gwbp_densify_emit(int64_t n, int64_t n_out, const uint8_t *kind, const int64_t *offsets, const float *means,
                               const float *scaling, const float *rotation, const float *opacity, const float *noise, float log16,
                               int32_t *parent, uint8_t *child, float *out_means, float *out_scaling, float *out_rotation,
                               float *out_opacity, void *stream);
GWBP_API int gwbp_densify_gather(int64_t n, int64_t n_out, int32_t w, const float *table, int64_t ldt, const int32_t *parent,
                                 const uint8_t *child, const uint8_t *kind, int32_t mode, float *out, int64_t ldo, void *stream);

/* ---- the MCMC strategy: relocation of dead Gaussians, growth to a cap, noise on the means (gsplat's MCMCStrategy) ----
 * All arrays are dense unless a stride is named; float32 unless a type is named.  No atomics: the same inputs give the same bits.
 * csrc/mcmc_math.h holds the expressions in their order.  n Gaussians, m draws.
 *
 * gwbp_mcmc_plan  weight[i] = floor(sigmoid(opacity[i]) 2^24) as int64, 0 where !(opacity[i] > t_opa) under GWBP_MCMC_RELOCATE (logits;
 *     a NaN is dead); under GWBP_MCMC_ADD only a NaN has weight 0.  dead[i] = !(opacity[i] > t_opa) in both modes.  cdf and dead_offsets
 *     (int64 [n + 1]) are the exclusive scans of the two, cdf[n] and dead_offsets[n] the totals; dead_idx (int32 [n]) holds the dead
 *     Gaussians in ascending order in its first dead_offsets[n] entries.  workspace: gwbp_mcmc_plan_workspace_size(n) bytes, 8-B
 *     aligned, free when the kernels have run.  n = 0 writes cdf[0] = dead_offsets[0] = 0.
 * gwbp_mcmc_draw  parent[j] (int32 [m]) = the i with cdf[i] <= t < cdf[i + 1], t = min((int64)(u[j] cdf[n]), cdf[n] - 1); u float64
 *     [m] in [0, 1), ASCENDING (then parent is ascending, which gwbp_mcmc_update needs).  cdf[n] = 0: parent[j] = -1.
 * gwbp_mcmc_update  count[i] (int32 [n]) = the number of draws of i.  Where it is positive, opacity[i] and scaling[i, 0..2] (row
 *     stride lds) become, IN PLACE and in pre-activation form, with r = min(count[i] + 1, GWBP_MCMC_MAX_RATIO):
 *         o' = 1 - (1 - o)^(1 / r), clamped to [min_opacity, 1 - 2^-23];   s' = s o / D(o', r)   (D of the unclamped o')
 * gwbp_mcmc_move  table[dead_idx[j], 0..w) = table[parent[j], 0..w) for j < m, IN PLACE (row stride ldt >= w).  A dead Gaussian is
 *     never a parent, so no row is both read and written; a pair with an index outside [0, n) moves nothing.
 * gwbp_mcmc_zero_rows  table[i, 0..w) = 0 where count[i] > 0, i < n (optimiser moments of the parents).
 * gwbp_mcmc_noise  (every training step)  means[i] += R diag(exp(2 scaling[i])) R^T (z[i] g scaler), R of rotation[i] / |rotation[i]|,
 *     g = 1 / (1 + exp(-100 ((1 - sigmoid(opacity[i])) - 0.995))); means [n, 3] in place, z [n, 3].
 * gwbp_mcmc_libm  out[i] = expf(a[i]), logf(a[i]) or powf(a[i], b[i]) as the kernels above evaluate them (b is read by POW only): what a
 *     test needs to hold them to a restatement bit for bit.
 * GWBP_EINVAL before any HIP call: n or m outside [0, 2^31 - 1], an unknown mode or op, w outside [1, GWBP_DENSIFY_MAX_WIDTH], a row
 * stride below its row, a min_opacity outside (0, 1), a null or misaligned array (4 B; cdf, dead_offsets, u and the workspace 8 B)
 * where n (m) > 0.  Whether u IS ascending cannot be seen on the host: the kernels check every row index instead.
 * GWBP_EWORKSPACE: a workspace below the size. */
#define GWBP_MCMC_RELOCATE 0
#define GWBP_MCMC_ADD 1
#define GWBP_MCMC_MAX_RATIO 51
#define GWBP_MCMC_LIBM_EXP 0
#define GWBP_MCMC_LIBM_LOG 1
#define GWBP_MCMC_LIBM_POW 2
GWBP_API int gwbp_mcmc_plan_workspace_size(int64_t n, size_t *bytes);
GWBP_API int gwbp_mcmc_plan(int64_t n, const float *opacity, float t_opa, int32_t mode, int64_t *cdf, int64_t *dead_offsets,
                            int32_t *dead_idx, void *workspace, size_t workspace_bytes, void *stream);
GWBP_API int gwbp_mcmc_draw(int64_t n, int64_t m, const int64_t *cdf, const double *u, int32_t *parent, void *stream);
GWBP_API int gwbp_mcmc_update(int64_t n, int64_t m, const int32_t *parent, float min_opacity, float *opacity, float *scaling,
                              int64_t lds, int32_t *count, void *stream);
GWBP_API int gwbp_mcmc_move(int64_t n, int64_t m, int32_t w, const int32_t *parent, const int32_t *dead_idx, float *table,
                            int64_t ldt, void *stream);
GWBP_API int gwbp_mcmc_zero_rows(int64_t n, int32_t w, const int32_t *count, float *table, int64_t ldt, void *stream);
GWBP_API int gwbp_mcmc_noise(int64_t n, float *means, const float *scaling, const float *rotation, const float *opacity,
                             const float *z, float scaler, void *stream);
GWBP_API int gwbp_mcmc_libm(int64_t n, int32_t op, const float *a, const float *b, float *out, void *stream);

/* ---- the optimiser step of training: Adam on one table, with an optional row mask (csrc/adam.hip) ----
 * gwbp_adam_step  p, m, v (float32 [n, w], dense, IN PLACE) from the gradient g [n, w], as torch.optim.Adam does with weight_decay = 0,
 *     amsgrad = False, maximize = False; csrc/adam_math.h holds the expressions in their order:
 *         m' = m + (1 - b1) (g - m);  v' = b2 v + ((1 - b2) g) g;  p' = p - lr_over_bc1 (m' / (sqrtf(v') / sqrt_bc2 + eps))
 *     lr_over_bc1 = lr / (1 - b1^t) and sqrt_bc2 = sqrt(1 - b2^t) of the step count t are the caller's, computed in float64 and rounded
 *     once; b1 and b2 are float64 so that 1 - b1 and 1 - b2 are formed there and rounded once.  Nothing is read back, nothing waits.
 *     visible == NULL: every row.  Otherwise uint8 [n]: row i is updated where visible[i] != 0, and the bits of p, m and v of every
 *     other row stay as they are; a 16-B chunk whose rows are all invisible is neither loaded nor stored.
 *     g == 0 where m == v == 0 leaves the bits of p, m and v (eps > 0).  No atomics: the same inputs give the same bits.
 * GWBP_EINVAL before any HIP call: n outside [0, 2^31 - 1], w < 1, a NaN lr_over_bc1, sqrt_bc2 <= 0, b1 or b2 outside [0, 1), eps < 0,
 * a null p, g, m or v where n > 0, one of them not 16-B aligned, p, m, v not distinct or one of them g or visible.  n = 0: nothing. */
GWBP_API int gwbp_adam_step(int64_t n, int32_t w, float *p, const float *g, float *m, float *v, const uint8_t *visible,
                            float lr_over_bc1, float sqrt_bc2, double b1, double b2, float eps, void *stream);

/* ---- depth supervision of training: the expected depth of a render against triangulated points or a depth map (csrc/depth_loss.hip;
 * DESIGN.md 4.0o; csrc/depth_math.h holds the expressions in their order) ----
 * render: float32 [height, width, Dp], dense, of an accumulated-depth mode (RGB+D, D): channel ch holds the accumulated depth A and is
 * read in place.  alpha: float32 [height, width], dense.  The expected depth of a pixel is e = A / max(alpha, 1e-10), +0 outside the
 * image.
 * gwbp_depth_points_loss      loss[0] (float32, device) = scale (sum_i t_i) / M over the M points (x_i, y_i) of points [M, 2] with
 *     true depths depths [M]: d_i the bilinear sample of e at column index x_i and row index y_i (column j is sampled at x = j, zero
 *     padding: the reference's grid_sample(align_corners=True) coordinates), q_i = d_i > 0 ? 1 / d_i : 0, t_i = |q_i - 1 / depths_i|.
 *     per_point: NULL, or float32 [M, 2] that takes (d_i, t_i).  M = 0: loss 0.  The sum is formed in float64 in a fixed order: the
 *     same inputs give the same bits.  workspace: GWBP_DEPTH_WORKSPACE_BYTES(M) bytes, 8-B aligned.
 * gwbp_depth_points_backward  ADDS upstream[0] * d loss / d render into channel ch of v_render [height, width, Dp] and
 *     upstream[0] * d loss / d alpha into v_alpha [height, width] (both zero-filled by the caller) with float atomics in an order that
 *     is not fixed: points share corners, the result is not bit-reproducible.  upstream: a float32 scalar ON THE DEVICE.  A sample with
 *     d_i <= 0 adds exact zeros (the torch expression gives NaN there), and so does M = 0.
 * gwbp_depth_map_loss         the same loss against a depth map depth [height, width] with optional weights [height, width] (NULL:
 *     all 1) over the valid pixels (depth > 0 and weight > 0): t = |q(e) - 1 / depth| (GWBP_DEPTH_KIND_DISPARITY) or |e - depth|
 *     (GWBP_DEPTH_KIND_DEPTH), loss[0] = scale (sum w t) / (sum w), 0 without a valid pixel; sums [2] (float64, device) takes the two
 *     sums.  workspace: GWBP_DEPTH_WORKSPACE_BYTES(height * width) bytes.
 * gwbp_depth_map_backward     STORES every element of v_render [height, width, Dp] (zeros outside channel ch) and of v_alpha: no
 *     atomics, the same bits every run.  sums: what the forward wrote.  A pixel with e <= 0 takes zeros.
 * Non-finite inputs and depths <= 0 of the point term are not masked: they propagate.
 * GWBP_EINVAL before any HIP call: height or width outside [1, 2^24] or more than 2^31 - 1 pixels, Dp < 1, ch outside [0, Dp), M outside [0, 2^31 - 1], an unknown
 * kind, a null or 4-B misaligned pointer (8-B: sums, workspace) among those the call reads or writes (points and depths may be NULL
 * when M = 0, and so may the workspace).  GWBP_EWORKSPACE: a workspace below the size above. */
#define GWBP_DEPTH_KIND_DISPARITY 0
#define GWBP_DEPTH_KIND_DEPTH 1
#define GWBP_DEPTH_BLOCK 256 /* points per workgroup of the point term */
#define GWBP_DEPTH_WORKSPACE_BYTES(n) ((((size_t)(n) + GWBP_DEPTH_BLOCK - 1) / GWBP_DEPTH_BLOCK) * 16)
GWBP_API int gwbp_depth_points_loss(int32_t height, int32_t width, int32_t Dp, int32_t ch, const float *render, const float *alpha,
                                    int64_t M, const float *points, const float *depths, float scale, float *loss, float *per_point,
                                    void *workspace, size_t workspace_bytes, void *stream);
GWBP_API int gwbp_depth_points_backward(int32_t height, int32_t width, int32_t Dp, int32_t ch, const float *render, const float *alpha,
                                        int64_t M, const float *points, const float *depths, float scale, const float *upstream,
                                        float *v_render, float *v_alpha, void *stream);
GWBP_API int gwbp_depth_map_loss(int32_t height, int32_t width, int32_t Dp, int32_t ch, const float *render, const float *alpha,
                                 const float *depth, const float *weights, int32_t kind, float scale, float *loss, double *sums,
                                 void *workspace, size_t workspace_bytes, void *stream);
GWBP_API int gwbp_depth_map_backward(int32_t height, int32_t width, int32_t Dp, int32_t ch, const float *render, const float *alpha,
                                     const float *depth, const float *weights, int32_t kind, float scale, const double *sums,
                                     const float *upstream, float *v_render, float *v_alpha, void *stream);

/* Adds this view's counters into `accum` (device, gwbp_stats) -- used by bench/driver to total pairs. */
GWBP_API int gwbp_accumulate_stats(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, gwbp_stats *accum,
                          void *stream);
/* Copies the workspace's counters of the last view to host memory.  SYNCHRONISES `stream`. */
GWBP_API int gwbp_read_stats(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, gwbp_stats *stats_host,
                    void *stream);

/* Debug/test: expand the sparse weight store of the last blended view into triples, sorted by nothing in
 * particular.  gid/pix/w have room for `cap` entries; *n_host receives the count.  SYNCHRONISES. */
GWBP_API int gwbp_dump_pairs(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                    int64_t cap, int32_t *gid, int32_t *pix, float *w, int64_t *n_host, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GWBP_H */
