// capi.hip -- extern "C" entry points of libgwbp.so (see include/gwbp.h for the contract).
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <mutex>

#include "gwbp_dev.h"
#include "mask_features.h"

namespace gwbp {

static thread_local char g_err[512] = "";

int set_error(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int check_hip(hipError_t e, const char *what)
{
    if (e == hipSuccess)
        return GWBP_OK;
    set_error((int)e, "%s: %s", what, hipGetErrorString(e));
    return (int)e;
}

namespace {
struct DevCache {
    int n_cu;                         // benign race: every writer stores the same value
    std::map<const void *, int> lds;  // kernel -> the largest dynamic-LDS limit set on this device (under g_lds_mutex)
};
DevCache g_dev[64];
// One lock for every device's map: launches come from a few host threads, so it is uncontended, and a lookup costs nanoseconds beside
// a launch's microseconds.  It is held across hipFuncSetAttribute on purpose, so that two threads never set one kernel's limit at once
// and the recorded size is the one in force.
std::mutex g_lds_mutex;
DevCache *dev_cache()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64)
        return nullptr;
    return &g_dev[dev];
}
} // namespace

int device_cus(int *n_cu)
{
    DevCache *c = dev_cache();
    if (!c)
        return set_error(GWBP_EINVAL, "cannot query the current device");
    if (c->n_cu == 0) {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
            return set_error(GWBP_EINVAL, "cannot query the device for the persistent scatter grid");
        c->n_cu = v > 0 ? v : 256;
    }
    *n_cu = c->n_cu;
    return GWBP_OK;
}

int ensure_dynamic_lds(const void *func, int bytes)
{
    DevCache *c = dev_cache();
    if (!c)
        return set_error(GWBP_EINVAL, "cannot query the current device");
    std::lock_guard<std::mutex> lock(g_lds_mutex);
    const auto it = c->lds.find(func);
    if (it != c->lds.end() && bytes <= it->second)
        return GWBP_OK;
    const int rc = check_hip(hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, bytes),
                             "dynamic LDS attribute");
    if (rc == GWBP_OK)
        c->lds[func] = bytes;
    return rc;
}

int profile_knob(const char *name)
{
#ifdef GWBP_PROFILE
    const char *v = getenv(name);
    return v ? atoi(v) : 0;
#else
    (void)name;
    return 0;
#endif
}

static size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

int make_layout(const gwbp_caps *c, Layout *L)
{
    if (!c || !L)
        return set_error(GWBP_EINVAL, "null caps");
    if (c->n_gaussians < 0 || c->n_gaussians > 0x7FFFFFFFll || c->isect_cap < 1 || c->isect_cap > 0xFFFFF000ll ||
        c->pair_cap < (int64_t)kPage * kShards || c->pair_cap > 0xFFFFF000ll || c->max_width < 1 || c->max_height < 1 ||
        c->max_width > 65535 * kTile || c->max_height > 65535 * kTile)
        return set_error(GWBP_EINVAL, "caps out of range (N=%lld isect_cap=%lld pair_cap=%lld %dx%d)",
                         (long long)c->n_gaussians, (long long)c->isect_cap, (long long)c->pair_cap, c->max_width,
                         c->max_height);
    if (c->flags & ~(GWBP_FLAG_TIGHT_BINNING | GWBP_FLAG_FRONT_PRIORITY | GWBP_FLAG_NARROW_SCATTER | GWBP_FLAG_SPLIT_ENCODER))
        return set_error(GWBP_EINVAL, "unknown caps.flags bits 0x%x", (unsigned)c->flags);
    memset(L, 0, sizeof(*L));
    L->n = c->n_gaussians;
    L->isect_cap = c->isect_cap;
    L->pair_cap = c->pair_cap;
    L->scatter_wgs = c->scatter_workgroups > 0 ? c->scatter_workgroups : 0;
    L->flags = c->flags;
    const int tw = (c->max_width + kTile - 1) / kTile, th = (c->max_height + kTile - 1) / kTile;
    L->max_tiles = tw * th;
    L->n_scan_blocks = (int)((L->n + kScanBlock - 1) / kScanBlock);
    L->n_sort_blocks = (int)(((L->isect_cap > L->n ? L->isect_cap : L->n) + kSortItems - 1) / kSortItems);
    size_t o = 0;
    auto take = [&](size_t bytes) {
        size_t at = o;
        o += align_up(bytes ? bytes : 1);
        return at;
    };
    L->counters = take(sizeof(Counters));
    L->shards = take((size_t)(kShards + kQueues) * 64);
    L->sweep = take((size_t)kSweepWords * sizeof(u32)); // (inside the range gwbp_project's memset clears: counters .. g2d)
    L->g2d = take((size_t)L->n * sizeof(G2D));
    L->rect = take((size_t)L->n * sizeof(uint2));
    L->touched = take((size_t)L->n * sizeof(u32));
    L->blocksums = take((size_t)(L->n_scan_blocks + 1) * sizeof(u32));
    for (int i = 0; i < 2; ++i) {
        L->dkeys[i] = take((size_t)L->n * sizeof(u32));
        L->dvals[i] = take((size_t)L->n * sizeof(u32));
    }
    L->keys[0] = take((size_t)L->isect_cap * sizeof(u32));
    L->keys[1] = take((size_t)L->isect_cap * sizeof(u32));
    L->vals[0] = take((size_t)L->isect_cap * sizeof(u32));
    L->vals[1] = take((size_t)L->isect_cap * sizeof(u32));
#ifdef GWBP_SORT_ONESWEEP
    // two look-back status buffers [block][256 digits] of 8-B words, used alternately by the passes of a sort level
    L->hist = take((size_t)2 * 256 * L->n_sort_blocks * sizeof(u64));
#else
    L->hist = take((size_t)256 * L->n_sort_blocks * sizeof(u32));
#endif
    L->digit_total = take(256 * sizeof(u32));
    L->tile_offsets = take((size_t)(L->max_tiles + 1) * sizeof(u32));
    L->tile_order = take((size_t)L->max_tiles * sizeof(u32));
    L->hdr_count = take((size_t)L->max_tiles * sizeof(u32));
    L->headers = take((size_t)L->isect_cap * sizeof(Header));
    L->carry = take((size_t)kCarryWgs * kCarryRows * 256 * sizeof(float));
    // + 128 entries of slack behind the pool: k_scatter_wide's L2 warm-up touches one dword per 128-B line of a visit's run and
    // may reach one line past its end (its scalar batch loads stay inside the record's padded lists), and k_render_rows4 reads
    // 16 entries from a visit's first one whatever the visit's length (15 entries = 120 B past the last record at most)
    L->wpool = take((size_t)L->pair_cap * sizeof(WPair) + 1024);
    L->total = o;
    return GWBP_OK;
}

int bind_workspace(const gwbp_caps *caps, void *ws, size_t bytes, Layout *L, Ws *W)
{
    int rc = make_layout(caps, L);
    if (rc)
        return rc;
    if (!ws)
        return set_error(GWBP_EINVAL, "null workspace");
    if ((reinterpret_cast<uintptr_t>(ws) & 255) != 0)
        return set_error(GWBP_EINVAL, "workspace must be 256-B aligned");
    if (bytes < L->total)
        return set_error(GWBP_EWORKSPACE, "workspace too small: have %zu, need %zu", bytes, L->total);
    char *b = static_cast<char *>(ws);
    W->counters = reinterpret_cast<Counters *>(b + L->counters);
    W->shards = reinterpret_cast<u32 *>(b + L->shards);
    W->sweep = reinterpret_cast<u32 *>(b + L->sweep);
    W->g2d = reinterpret_cast<G2D *>(b + L->g2d);
    W->rect = reinterpret_cast<uint2 *>(b + L->rect);
    W->touched = reinterpret_cast<u32 *>(b + L->touched);
    W->blocksums = reinterpret_cast<u32 *>(b + L->blocksums);
    for (int i = 0; i < 2; ++i) {
        W->dkeys[i] = reinterpret_cast<u32 *>(b + L->dkeys[i]);
        W->dvals[i] = reinterpret_cast<u32 *>(b + L->dvals[i]);
    }
    W->keys[0] = reinterpret_cast<u32 *>(b + L->keys[0]);
    W->keys[1] = reinterpret_cast<u32 *>(b + L->keys[1]);
    W->vals[0] = reinterpret_cast<u32 *>(b + L->vals[0]);
    W->vals[1] = reinterpret_cast<u32 *>(b + L->vals[1]);
    W->hist = reinterpret_cast<u32 *>(b + L->hist);
    W->digit_total = reinterpret_cast<u32 *>(b + L->digit_total);
    W->tile_offsets = reinterpret_cast<u32 *>(b + L->tile_offsets);
    W->tile_order = reinterpret_cast<u32 *>(b + L->tile_order);
    W->hdr_count = reinterpret_cast<u32 *>(b + L->hdr_count);
    W->headers = reinterpret_cast<Header *>(b + L->headers);
    W->carry = reinterpret_cast<float *>(b + L->carry);
    W->wpool = reinterpret_cast<WPair *>(b + L->wpool);
    return GWBP_OK;
}

int make_view(const gwbp_view *v, const gwbp_caps *caps, ViewDev *o)
{
    if (!v)
        return set_error(GWBP_EINVAL, "null view");
    if (v->width < 1 || v->height < 1 || v->width > caps->max_width || v->height > caps->max_height)
        return set_error(GWBP_EINVAL, "view %dx%d outside caps %dx%d", v->width, v->height, caps->max_width,
                         caps->max_height);
    const int tw = (v->width + kTile - 1) / kTile, th = (v->height + kTile - 1) / kTile;
    const int max_tiles = ((caps->max_width + kTile - 1) / kTile) * ((caps->max_height + kTile - 1) / kTile);
    if (tw * th > max_tiles)
        return set_error(GWBP_EINVAL, "view has more tiles than the caps allow");
    if (!(v->K[0] > 0.f) || !(v->K[4] > 0.f))
        return set_error(GWBP_EINVAL, "focal lengths must be positive");
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c)
            o->R[3 * r + c] = v->viewmat[4 * r + c];
        o->t[r] = v->viewmat[4 * r + 3];
    }
    o->fx = v->K[0], o->fy = v->K[4], o->cx = v->K[2], o->cy = v->K[5];
    o->W = v->width, o->H = v->height, o->tile_w = tw, o->tile_h = th;
    o->near_plane = v->near_plane, o->far_plane = v->far_plane, o->eps2d = v->eps2d, o->radius_clip = v->radius_clip;
    return GWBP_OK;
}

static int check_feats(const float *feats, int64_t fs_y, int64_t fs_x, int64_t fs_c, int D)
{
    if (!feats || D < 1 || fs_y < 0 || fs_x < 0 || fs_c < 0)
        return set_error(GWBP_EINVAL, "bad feature map arguments (D=%d strides %lld %lld %lld)", D, (long long)fs_y,
                         (long long)fs_x, (long long)fs_c);
    return GWBP_OK;
}

// gwbp_pixel_weights -> PixW; NULL -> no map.  Checked before anything else of an _ex call.
static int check_pixel_weights(const gwbp_pixel_weights *pw, PixW *out, const PixW **use)
{
    *use = nullptr;
    if (!pw)
        return GWBP_OK;
    if (pw->dtype != GWBP_PIXW_F32 && pw->dtype != GWBP_PIXW_F16 && pw->dtype != GWBP_PIXW_BF16 && pw->dtype != GWBP_PIXW_U8)
        return set_error(GWBP_EINVAL, "unknown pixel weight type %d", (int)pw->dtype);
    if (!pw->data)
        return set_error(GWBP_EINVAL, "null pixel weight map");
    if (pw->ws_y < 0 || pw->ws_x < 0)
        return set_error(GWBP_EINVAL, "negative pixel weight strides (%lld %lld)", (long long)pw->ws_y, (long long)pw->ws_x);
    if (pw->reserved != 0)
        return set_error(GWBP_EINVAL, "gwbp_pixel_weights.reserved must be 0 (got %d)", (int)pw->reserved);
    out->data = pw->data, out->ws_y = pw->ws_y, out->ws_x = pw->ws_x, out->dtype = pw->dtype;
    *use = out;
    return GWBP_OK;
}

} // namespace gwbp

using namespace gwbp;
static_assert(sizeof(gwbp_pixel_weights) == 32, "gwbp_pixel_weights is part of the ABI");
// the rows' partial sums of gwbp_field_compare live in the carry slices (field_compare.hip)
static_assert((size_t)GWBP_FIELD_COMPARE_MAX_TILES * 16 * 6 * sizeof(double) <= (size_t)kCarryWgs * kCarryRows * 256 * sizeof(float),
              "GWBP_FIELD_COMPARE_MAX_TILES does not fit the carry slices");

static hipStream_t as_stream(void *stream) { return static_cast<hipStream_t>(stream); }

// One call on one view of a workspace: what every launcher of such a call takes.
struct Bound {
    Layout L;
    Ws W;
    ViewDev V;
    hipStream_t s;
};

// The caps, then the workspace, then the view: the order include/gwbp.h gives for them.
static int bind(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host, void *stream,
                Bound *B)
{
    int rc = bind_workspace(caps, workspace, workspace_bytes, &B->L, &B->W);
    if (rc)
        return rc;
    B->s = as_stream(stream);
    return make_view(view_host, caps, &B->V);
}

// The RGB composite of the gwbp_blend_*_rgb forms: both pointers or neither (*use = nullptr: the _ex function).
static int check_rgb(const float *colors, float *image, RgbOut *out, const RgbOut **use)
{
    *use = nullptr;
    if (!colors && !image)
        return GWBP_OK;
    if (!colors || !image)
        return set_error(GWBP_EINVAL, "the RGB composite needs both colors [N,3] and image [H,W,3] (got %s colors, %s image)",
                         colors ? "a" : "null", image ? "an" : "null");
    out->colors = colors, out->image = image;
    *use = out;
    return GWBP_OK;
}

// The pixel-weight map and the RGB composite of the three _rgb blends, checked in that order before anything else.
struct BlendExtras {
    PixW P;
    RgbOut R;
    const PixW *pw;
    const RgbOut *rgb;
};

static int check_blend_extras(const gwbp_pixel_weights *pixel_weights, const float *colors, float *image, BlendExtras *X)
{
    const int rc = check_pixel_weights(pixel_weights, &X->P, &X->pw);
    return rc ? rc : check_rgb(colors, image, &X->R, &X->rgb);
}

static bool known_map_type(int32_t mt) { return mt == GWBP_MAP_F32 || mt == GWBP_MAP_F16 || mt == GWBP_MAP_BF16; }

// The element type of a finished field handed to a *_typed entry point (or of gwbp_finalize_typed's output): checked before anything else.
static int check_field_type(const char *what, int32_t field_type)
{
    if (!known_map_type(field_type))
        return set_error(GWBP_EINVAL, "%s: unknown field_type %d (GWBP_MAP_F32, GWBP_MAP_F16 or GWBP_MAP_BF16)", what, (int)field_type);
    return GWBP_OK;
}
// A field pointer that is not aligned to its element.  The fp32 case stays with each entry point's own check and message (fp32_off
// is then part of that check's condition); a half field (2-B elements) is refused here.
static bool fp32_off(const void *p, int32_t field_type)
{
    return field_type == GWBP_MAP_F32 && (reinterpret_cast<uintptr_t>(p) & 3) != 0;
}
static int check_half_alignment(const char *what, const char *name, const void *p, int32_t field_type)
{
    if (field_type != GWBP_MAP_F32 && (reinterpret_cast<uintptr_t>(p) & 1))
        return set_error(GWBP_EINVAL, "%s: a half %s must be 2-B aligned", what, name);
    return GWBP_OK;
}

static int check_label_type(int32_t label_type)
{
    if (label_type != GWBP_LABEL_U8 && label_type != GWBP_LABEL_I16 && label_type != GWBP_LABEL_I32)
        return set_error(GWBP_EINVAL, "unknown label type %d", (int)label_type);
    return GWBP_OK;
}

static int check_index_maps(const char *fn, const int32_t *ymap, const int32_t *xmap)
{
    if (!ymap != !xmap)
        return set_error(GWBP_EINVAL, "%s needs both index maps or neither", fn);
    return GWBP_OK;
}

static int check_label_map(const void *labels, int64_t ls_y, int64_t ls_x)
{
    if (!labels || ls_y < 0 || ls_x < 0)
        return set_error(GWBP_EINVAL, "bad label map arguments (strides %lld %lld)", (long long)ls_y, (long long)ls_x);
    return GWBP_OK;
}

// The label map and the [N, num_classes] accumulator (F of gwbp_scatter_labels, C of the votes; `acc` and `ld` are its name and
// its leading dimension's in the messages), checked before the caps, the workspace or the view.
static int check_label_args(const char *fn, const void *labels, int32_t label_type, int64_t ls_y, int64_t ls_x, const int32_t *ymap,
                            const int32_t *xmap, int32_t num_classes, const char *acc, const float *A, const char *ld, int64_t lda)
{
    int rc = check_label_type(label_type);
    if (rc)
        return rc;
    if (num_classes <= 0)
        return set_error(GWBP_EINVAL, "num_classes must be positive (got %d)", (int)num_classes);
    if (lda < num_classes)
        return set_error(GWBP_EINVAL, "%s %lld < num_classes %d", ld, (long long)lda, (int)num_classes);
    if (!A)
        return set_error(GWBP_EINVAL, "null %s", acc);
    if ((rc = check_index_maps(fn, ymap, xmap)))
        return rc;
    return check_label_map(labels, ls_y, ls_x);
}

// The label map, the int32 table (`aux`: group of gwbp_label_overlap, remap of gwbp_label_votes) and the int64 accumulator of the
// two association walks (`acc` and `ld` are its name and its leading dimension's in the messages).
static int check_assoc_args(const char *fn, const void *labels, int32_t label_type, int64_t ls_y, int64_t ls_x, const int32_t *ymap,
                            const int32_t *xmap, int32_t num_labels, const char *aux_name, const int32_t *aux, int32_t n_cols,
                            const char *acc, const int64_t *A, const char *ld, int64_t lda)
{
    int rc = check_label_type(label_type);
    if (rc)
        return rc;
    if (num_labels <= 0)
        return set_error(GWBP_EINVAL, "num_labels must be positive (got %d)", (int)num_labels);
    if (n_cols <= 0)
        return set_error(GWBP_EINVAL, "n_cols must be positive (got %d)", (int)n_cols);
    if (lda < n_cols)
        return set_error(GWBP_EINVAL, "%s %lld < n_cols %d", ld, (long long)lda, (int)n_cols);
    if (!aux)
        return set_error(GWBP_EINVAL, "null %s", aux_name);
    if (!A || (reinterpret_cast<uintptr_t>(A) & 7))
        return set_error(GWBP_EINVAL, "%s must be a non-null, 8-B aligned int64 array", acc);
    if ((rc = check_index_maps(fn, ymap, xmap)))
        return rc;
    return check_label_map(labels, ls_y, ls_x);
}

// The slot lists of gwbp_label_votes_sparse over n rows: each array present and aligned, the row strides, and no two of the byte
// ranges the kernel may write overlapping each other.
static int check_sparse_lists(int64_t n, int32_t slots, const int32_t *keys, int64_t ld_keys, const int64_t *vals, int64_t ld_vals,
                              const int64_t *spill, const int64_t *total)
{
    if (slots < 1 || slots > GWBP_SPARSE_MAX_SLOTS)
        return set_error(GWBP_EINVAL, "slots must lie in [1, %d] (got %d)", GWBP_SPARSE_MAX_SLOTS, (int)slots);
    if (ld_keys < slots)
        return set_error(GWBP_EINVAL, "ld_keys %lld < slots %d", (long long)ld_keys, (int)slots);
    if (ld_vals < slots)
        return set_error(GWBP_EINVAL, "ld_vals %lld < slots %d", (long long)ld_vals, (int)slots);
    if (!keys || (reinterpret_cast<uintptr_t>(keys) & 3))
        return set_error(GWBP_EINVAL, "keys must be a non-null, 4-B aligned int32 array");
    if (!vals || (reinterpret_cast<uintptr_t>(vals) & 7))
        return set_error(GWBP_EINVAL, "vals must be a non-null, 8-B aligned int64 array");
    if (!spill || (reinterpret_cast<uintptr_t>(spill) & 7))
        return set_error(GWBP_EINVAL, "spill must be a non-null, 8-B aligned int64 array");
    if (reinterpret_cast<uintptr_t>(total) & 7)
        return set_error(GWBP_EINVAL, "total must be an 8-B aligned int64 array (or NULL)");
    const uint64_t rows = n > 0 ? (uint64_t)n : 0u;
    const uint64_t span = rows ? rows - 1u : 0u; // (a list of n rows ends `slots` elements into its last row)
    struct Range {
        const char *name;
        uintptr_t lo;
        uint64_t bytes;
    } r[4] = {{"keys", reinterpret_cast<uintptr_t>(keys), rows ? (span * (uint64_t)ld_keys + (uint64_t)slots) * 4u : 0u},
              {"vals", reinterpret_cast<uintptr_t>(vals), rows ? (span * (uint64_t)ld_vals + (uint64_t)slots) * 8u : 0u},
              {"spill", reinterpret_cast<uintptr_t>(spill), rows * 8u},
              {"total", reinterpret_cast<uintptr_t>(total), total ? rows * 8u : 0u}};
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j)
            if (r[i].bytes && r[j].bytes && r[i].lo < r[j].lo + r[j].bytes && r[j].lo < r[i].lo + r[i].bytes)
                return set_error(GWBP_EINVAL, "%s and %s overlap", r[i].name, r[j].name);
    return GWBP_OK;
}

extern "C" {

const char *gwbp_version(void)
{
#ifdef GWBP_PROFILE
    return "libgwbp gfx950 r6 (PROFILE build: ablation knobs live, results may be invalid)";
#else
    return "libgwbp gfx950 r6";
#endif
}
const char *gwbp_last_error_string(void) { return g_err; }

int gwbp_workspace_size(const gwbp_caps *caps, size_t *bytes_host)
{
    Layout L;
    int rc = make_layout(caps, &L);
    if (rc)
        return rc;
    if (!bytes_host)
        return set_error(GWBP_EINVAL, "null bytes_host");
    *bytes_host = L.total;
    return GWBP_OK;
}

int gwbp_project(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                 const float *means, const float *quats, const float *scales, const float *opacities,
                 int32_t *radii, float *means2d, float *depths, float *conics, void *stream)
{
    return gwbp_project_camera(caps, workspace, workspace_bytes, view_host, GWBP_CAMERA_PINHOLE, GWBP_RASTERIZE_CLASSIC,
                               means, quats, scales, opacities, radii, means2d, depths, conics, nullptr, stream);
}

int gwbp_project_camera(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                        int32_t camera_model, int32_t rasterize_mode, const float *means, const float *quats,
                        const float *scales, const float *opacities, int32_t *radii, float *means2d, float *depths,
                        float *conics, float *compensations, void *stream)
{
    // validated before anything touches the device
    if (camera_model != GWBP_CAMERA_PINHOLE && camera_model != GWBP_CAMERA_ORTHO && camera_model != GWBP_CAMERA_FISHEYE)
        return set_error(GWBP_EINVAL, "unknown camera model %d", (int)camera_model);
    if (rasterize_mode != GWBP_RASTERIZE_CLASSIC && rasterize_mode != GWBP_RASTERIZE_ANTIALIASED)
        return set_error(GWBP_EINVAL, "unknown rasterize mode %d", (int)rasterize_mode);
    Bound B;
    int rc = bind(caps, workspace, workspace_bytes, view_host, stream, &B);
    if (rc)
        return rc;
    if (B.L.n > 0 && (!means || !quats || !scales || !opacities))
        return set_error(GWBP_EINVAL, "null Gaussian parameter pointer");
    if (reinterpret_cast<uintptr_t>(quats) & 15)
        return set_error(GWBP_EINVAL, "quats must be 16-B aligned");
    return launch_project(B.L, B.W, B.V, means, quats, scales, opacities, radii, means2d, depths, conics, B.s, camera_model,
                          rasterize_mode, compensations);
}

int gwbp_bin_sort(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                  int64_t *isect_ids, int32_t *flatten_ids, int32_t *tile_offsets, void *stream)
{
    Bound B;
    int rc = bind(caps, workspace, workspace_bytes, view_host, stream, &B);
    if (rc)
        return rc;
    return launch_bin_sort(B.L, B.W, B.V, isect_ids, flatten_ids, tile_offsets, B.s);
}

int gwbp_blend_weights(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                       float *alphas, void *stream)
{
    return gwbp_blend_weights_ex(caps, workspace, workspace_bytes, view_host, alphas, nullptr, stream);
}

int gwbp_blend_weights_ex(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                          float *alphas, const gwbp_pixel_weights *pixel_weights, void *stream)
{
    return gwbp_blend_weights_rgb(caps, workspace, workspace_bytes, view_host, alphas, pixel_weights, nullptr, nullptr, stream);
}

int gwbp_blend_weights_rgb(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                           float *alphas, const gwbp_pixel_weights *pixel_weights, const float *colors, float *image,
                           void *stream)
{
    BlendExtras X;
    int rc = check_blend_extras(pixel_weights, colors, image, &X);
    if (rc)
        return rc;
    Bound B;
    if ((rc = bind(caps, workspace, workspace_bytes, view_host, stream, &B)))
        return rc;
    return launch_blend(B.L, B.W, B.V, alphas, nullptr, 0.f, B.s, nullptr, 0, 1.0f, nullptr, X.pw, X.rgb);
}

int gwbp_blend_weights_d(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                         float *alphas, float scale_d, float *d, void *stream)
{
    return gwbp_blend_weights_d_ex(caps, workspace, workspace_bytes, view_host, alphas, scale_d, d, nullptr, stream);
}

int gwbp_blend_weights_d_ex(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                            float *alphas, float scale_d, float *d, const gwbp_pixel_weights *pixel_weights, void *stream)
{
    return gwbp_blend_weights_d_rgb(caps, workspace, workspace_bytes, view_host, alphas, scale_d, d, pixel_weights, nullptr,
                                    nullptr, stream);
}

int gwbp_blend_weights_d_rgb(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                             float *alphas, float scale_d, float *d, const gwbp_pixel_weights *pixel_weights,
                             const float *colors, float *image, void *stream)
{
    BlendExtras X;
    int rc = check_blend_extras(pixel_weights, colors, image, &X);
    if (rc)
        return rc;
    Bound B;
    if ((rc = bind(caps, workspace, workspace_bytes, view_host, stream, &B)))
        return rc;
    if (!d)
        return set_error(GWBP_EINVAL, "null d");
    return launch_blend(B.L, B.W, B.V, alphas, d, scale_d, B.s, nullptr, 0, 1.0f, nullptr, X.pw, X.rgb);
}

int gwbp_blend_scatter(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                       const float *feats, int64_t fs_y, int64_t fs_x, int32_t D, float scale_f, float scale_d, float *F,
                       float *d, float *alphas, void *stream)
{
    return gwbp_blend_scatter_ex(caps, workspace, workspace_bytes, view_host, feats, fs_y, fs_x, D, scale_f, scale_d, F, d, alphas,
                                 nullptr, stream);
}

int gwbp_blend_scatter_ex(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                          const float *feats, int64_t fs_y, int64_t fs_x, int32_t D, float scale_f, float scale_d, float *F,
                          float *d, float *alphas, const gwbp_pixel_weights *pixel_weights, void *stream)
{
    PixW P;
    const PixW *pw;
    int rc = check_pixel_weights(pixel_weights, &P, &pw);
    if (rc)
        return rc;
    Bound B;
    if ((rc = bind(caps, workspace, workspace_bytes, view_host, stream, &B)))
        return rc;
    const FeatMap M{feats, fs_y, fs_x, 1, nullptr, nullptr, nullptr, nullptr, 0, 0};
    return launch_blend(B.L, B.W, B.V, alphas, d, scale_d, B.s, &M, D, scale_f, F, pw);
}

int gwbp_blend_scatter_encoded(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                               const float *feats, int64_t fs_y, int64_t fs_x, int32_t K, const float *encoder, int32_t n_out,
                               float scale_f, float scale_d, float *F, float *d, float *alphas, void *stream)
{
    return gwbp_blend_scatter_encoded_ex(caps, workspace, workspace_bytes, view_host, feats, fs_y, fs_x, K, encoder, n_out, scale_f,
                                         scale_d, F, d, alphas, nullptr, stream);
}

int gwbp_blend_scatter_encoded_ex(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                                  const float *feats, int64_t fs_y, int64_t fs_x, int32_t K, const float *encoder, int32_t n_out,
                                  float scale_f, float scale_d, float *F, float *d, float *alphas,
                                  const gwbp_pixel_weights *pixel_weights, void *stream)
{
    PixW P;
    const PixW *pw;
    int rc = check_pixel_weights(pixel_weights, &P, &pw);
    if (rc)
        return rc;
    Bound B;
    if ((rc = bind(caps, workspace, workspace_bytes, view_host, stream, &B)))
        return rc;
    if (!encoder)
        return set_error(GWBP_EINVAL, "null encoder");
    FeatMap M{feats, fs_y, fs_x, 1, nullptr, nullptr, nullptr, nullptr, 0, 0};
    M.enc = encoder, M.enc_k = K;
    return launch_blend(B.L, B.W, B.V, alphas, d, scale_d, B.s, &M, n_out, scale_f, F, pw);
}

int gwbp_blend_tokens(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                      const int32_t *ymap, const int32_t *xmap, float *alphas, void *stream)
{
    return gwbp_blend_tokens_ex(caps, workspace, workspace_bytes, view_host, ymap, xmap, alphas, nullptr, stream);
}

int gwbp_blend_tokens_ex(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                         const int32_t *ymap, const int32_t *xmap, float *alphas, const gwbp_pixel_weights *pixel_weights,
                         void *stream)
{
    return gwbp_blend_tokens_rgb(caps, workspace, workspace_bytes, view_host, ymap, xmap, alphas, pixel_weights, nullptr, nullptr,
                                 stream);
}

int gwbp_blend_tokens_rgb(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                          const int32_t *ymap, const int32_t *xmap, float *alphas, const gwbp_pixel_weights *pixel_weights,
                          const float *colors, float *image, void *stream)
{
    BlendExtras X;
    int rc = check_blend_extras(pixel_weights, colors, image, &X);
    if (rc)
        return rc;
    Bound B;
    if ((rc = bind(caps, workspace, workspace_bytes, view_host, stream, &B)))
        return rc;
    return launch_blend_tokens(B.L, B.W, B.V, alphas, ymap, xmap, B.s, X.pw, X.rgb);
}

// gwbp_scatter_tokens and its typed form.  (The token pointer travels as it is; only the kernels of the map type dereference it.)
static int scatter_tokens(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                          const void *tokens, int mt, int64_t ts_y, int64_t ts_x, int32_t D, const int32_t *ymap,
                          const int32_t *xmap, float scale_f, float scale_d, float *F, float *d, void *stream)
{
    Bound B;
    int rc = bind(caps, workspace, workspace_bytes, view_host, stream, &B);
    if (rc)
        return rc;
    if (mt == GWBP_MAP_F32)
        return launch_token_apply(B.L, B.W, B.V, static_cast<const float *>(tokens), ts_y, ts_x, D, ymap, xmap, scale_f, scale_d, F,
                                  d, B.s);
    return launch_token_apply_half(B.L, B.W, B.V, tokens, ts_y, ts_x, D, ymap, xmap, scale_f, scale_d, F, d, B.s, mt);
}

int gwbp_scatter_tokens(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                        const float *tokens, int64_t ts_y, int64_t ts_x, int32_t D, const int32_t *ymap, const int32_t *xmap,
                        float scale_f, float scale_d, float *F, float *d, void *stream)
{
    return scatter_tokens(caps, workspace, workspace_bytes, view_host, tokens, GWBP_MAP_F32, ts_y, ts_x, D, ymap, xmap, scale_f,
                          scale_d, F, d, stream);
}

int gwbp_accumulate_d(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                      float scale_d, float *d, void *stream)
{
    Bound B;
    int rc = bind(caps, workspace, workspace_bytes, view_host, stream, &B);
    if (rc)
        return rc;
    if (!d)
        return set_error(GWBP_EINVAL, "null d");
    return launch_accum_d(B.L, B.W, B.V, scale_d, d, B.s);
}

// The scatter family.  Each form (plain, upsampled, bilinear) has ONE function that runs its pointer checks, in the name `fn` of
// the entry point that was called, and builds its FeatMap; the untyped entry point is its GWBP_MAP_F32 call.  (The feature
// pointer travels in FeatMap::p as it is; only the kernels of the map type dereference it.)
static int scatter_impl(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                        const FeatMap &M, int32_t D, float scale_f, float scale_d, float *F, float *d, void *stream,
                        int mt = GWBP_MAP_F32)
{
    Bound B;
    int rc = bind(caps, workspace, workspace_bytes, view_host, stream, &B);
    if (rc)
        return rc;
    if ((rc = check_feats(M.p, M.fs_y, M.fs_x, M.fs_c, D)))
        return rc;
    if (!F && B.L.n > 0)
        return set_error(GWBP_EINVAL, "null F");
    return launch_scatter(B.L, B.W, B.V, M, D, scale_f, scale_d, F, d, B.s, mt);
}

static int scatter_plain(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                         const void *feats, int mt, int64_t fs_y, int64_t fs_x, int64_t fs_c, int32_t D, float scale_f,
                         float scale_d, float *F, float *d, void *stream)
{
    const FeatMap M{static_cast<const float *>(feats), fs_y, fs_x, fs_c, nullptr, nullptr, nullptr, nullptr, 0, 0};
    return scatter_impl(caps, workspace, workspace_bytes, view_host, M, D, scale_f, scale_d, F, d, stream, mt);
}

static int scatter_upsampled(const char *fn, const gwbp_caps *caps, void *workspace, size_t workspace_bytes,
                             const gwbp_view *view_host, const void *feats, int mt, int64_t fs_y, int64_t fs_x, int64_t fs_c,
                             int32_t D, const int32_t *ymap, const int32_t *xmap, float scale_f, float scale_d, float *F, float *d,
                             void *stream)
{
    if (!ymap || !xmap)
        return set_error(GWBP_EINVAL, "%s needs both index maps", fn);
    const FeatMap M{static_cast<const float *>(feats), fs_y, fs_x, fs_c, ymap, xmap, nullptr, nullptr, 0, 0};
    return scatter_impl(caps, workspace, workspace_bytes, view_host, M, D, scale_f, scale_d, F, d, stream, mt);
}

static int scatter_bilinear(const char *fn, const gwbp_caps *caps, void *workspace, size_t workspace_bytes,
                            const gwbp_view *view_host, const void *feats, int mt, int64_t fs_y, int64_t fs_x, int64_t fs_c,
                            int32_t D, int32_t lr_h, int32_t lr_w, const int32_t *y0, const float *ly, const int32_t *x0,
                            const float *lx, float scale_f, float scale_d, float *F, float *d, void *stream)
{
    if (!y0 || !x0 || !ly || !lx || lr_h < 1 || lr_w < 1)
        return set_error(GWBP_EINVAL, "%s needs both index maps, both weight maps and the map size", fn);
    const FeatMap M{static_cast<const float *>(feats), fs_y, fs_x, fs_c, y0, x0, ly, lx, lr_h, lr_w};
    return scatter_impl(caps, workspace, workspace_bytes, view_host, M, D, scale_f, scale_d, F, d, stream, mt);
}

int gwbp_scatter(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                 const float *feats, int64_t fs_y, int64_t fs_x, int64_t fs_c, int32_t D, float scale_f,
                 float scale_d, float *F, float *d, void *stream)
{
    return scatter_plain(caps, workspace, workspace_bytes, view_host, feats, GWBP_MAP_F32, fs_y, fs_x, fs_c, D, scale_f, scale_d, F,
                         d, stream);
}

int gwbp_scatter_encoded(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                         const float *feats, int64_t fs_y, int64_t fs_x, int32_t K, const float *encoder, int32_t D,
                         float scale_f, float scale_d, float *F, float *d, void *stream)
{
    if (!encoder)
        return set_error(GWBP_EINVAL, "gwbp_scatter_encoded needs the encoder");
    FeatMap M{feats, fs_y, fs_x, 1, nullptr, nullptr, nullptr, nullptr, 0, 0};
    M.enc = encoder, M.enc_k = K;
    return scatter_impl(caps, workspace, workspace_bytes, view_host, M, D, scale_f, scale_d, F, d, stream);
}

int gwbp_scatter_upsampled(const gwbp_caps *caps, void *workspace, size_t workspace_bytes,
                           const gwbp_view *view_host, const float *feats, int64_t fs_y, int64_t fs_x, int64_t fs_c,
                           int32_t D, const int32_t *ymap, const int32_t *xmap, float scale_f, float scale_d, float *F,
                           float *d, void *stream)
{
    return scatter_upsampled("gwbp_scatter_upsampled", caps, workspace, workspace_bytes, view_host, feats, GWBP_MAP_F32, fs_y, fs_x,
                             fs_c, D, ymap, xmap, scale_f, scale_d, F, d, stream);
}

int gwbp_scatter_bilinear(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                          const float *feats, int64_t fs_y, int64_t fs_x, int64_t fs_c, int32_t D, int32_t lr_h,
                          int32_t lr_w, const int32_t *y0, const float *ly, const int32_t *x0, const float *lx,
                          float scale_f, float scale_d, float *F, float *d, void *stream)
{
    return scatter_bilinear("gwbp_scatter_bilinear", caps, workspace, workspace_bytes, view_host, feats, GWBP_MAP_F32, fs_y, fs_x,
                            fs_c, D, lr_h, lr_w, y0, ly, x0, lx, scale_f, scale_d, F, d, stream);
}

// The typed entry points: the map type is validated before anything else; GWBP_MAP_F32 is the untyped function's call, with
// that function's name in its messages.
int gwbp_scatter_typed(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                       const void *feats, int32_t map_type, int64_t fs_y, int64_t fs_x, int64_t fs_c, int32_t D, float scale_f,
                       float scale_d, float *F, float *d, void *stream)
{
    if (!known_map_type(map_type))
        return set_error(GWBP_EINVAL, "unknown map type %d", (int)map_type);
    return scatter_plain(caps, workspace, workspace_bytes, view_host, feats, map_type, fs_y, fs_x, fs_c, D, scale_f, scale_d, F, d,
                         stream);
}

int gwbp_scatter_upsampled_typed(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                                 const void *feats, int32_t map_type, int64_t fs_y, int64_t fs_x, int64_t fs_c, int32_t D,
                                 const int32_t *ymap, const int32_t *xmap, float scale_f, float scale_d, float *F, float *d,
                                 void *stream)
{
    if (!known_map_type(map_type))
        return set_error(GWBP_EINVAL, "unknown map type %d", (int)map_type);
    return scatter_upsampled(map_type == GWBP_MAP_F32 ? "gwbp_scatter_upsampled" : "gwbp_scatter_upsampled_typed", caps, workspace,
                             workspace_bytes, view_host, feats, map_type, fs_y, fs_x, fs_c, D, ymap, xmap, scale_f, scale_d, F, d,
                             stream);
}

int gwbp_scatter_bilinear_typed(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                                const void *feats, int32_t map_type, int64_t fs_y, int64_t fs_x, int64_t fs_c, int32_t D,
                                int32_t lr_h, int32_t lr_w, const int32_t *y0, const float *ly, const int32_t *x0,
                                const float *lx, float scale_f, float scale_d, float *F, float *d, void *stream)
{
    if (!known_map_type(map_type))
        return set_error(GWBP_EINVAL, "unknown map type %d", (int)map_type);
    return scatter_bilinear(map_type == GWBP_MAP_F32 ? "gwbp_scatter_bilinear" : "gwbp_scatter_bilinear_typed", caps, workspace,
                            workspace_bytes, view_host, feats, map_type, fs_y, fs_x, fs_c, D, lr_h, lr_w, y0, ly, x0, lx, scale_f,
                            scale_d, F, d, stream);
}

int gwbp_scatter_tokens_typed(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                              const void *tokens, int32_t map_type, int64_t ts_y, int64_t ts_x, int32_t D, const int32_t *ymap,
                              const int32_t *xmap, float scale_f, float scale_d, float *F, float *d, void *stream)
{
    if (!known_map_type(map_type))
        return set_error(GWBP_EINVAL, "unknown map type %d", (int)map_type);
    return scatter_tokens(caps, workspace, workspace_bytes, view_host, tokens, map_type, ts_y, ts_x, D, ymap, xmap, scale_f, scale_d,
                          F, d, stream);
}

int gwbp_scatter_labels(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                        const void *labels, int32_t label_type, int64_t ls_y, int64_t ls_x, int32_t num_classes,
                        const int32_t *ymap, const int32_t *xmap, float scale_f, float scale_d, float *F, int64_t ldf, float *d,
                        void *stream)
{
    // the label arguments first: nothing of the caps, the workspace or the view is looked at before they pass
    int rc = check_label_args("gwbp_scatter_labels", labels, label_type, ls_y, ls_x, ymap, xmap, num_classes, "F", F, "ldf", ldf);
    if (rc)
        return rc;
    Bound B;
    if ((rc = bind(caps, workspace, workspace_bytes, view_host, stream, &B)))
        return rc;
    return launch_scatter_labels(B.L, B.W, B.V, labels, label_type, ls_y, ls_x, ymap, xmap, num_classes, scale_f, scale_d, F, ldf, d,
                                 B.s);
}

int gwbp_scatter_mask_features(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                               const void *labels, int32_t label_type, int64_t ls_y, int64_t ls_x, const int32_t *ymap,
                               const int32_t *xmap, const void *table, int32_t table_type, int64_t ts_row, int32_t num_masks,
                               int32_t D, float scale_f, float scale_d, float *F, float *d, void *slots, size_t slots_bytes,
                               uint32_t *n_spilled, void *stream)
{
    // the map, table and slot arguments first: nothing of the workspace or the view is looked at before they pass
    int rc = check_label_type(label_type);
    if (rc)
        return rc;
    if (!known_map_type(table_type))
        return set_error(GWBP_EINVAL, "unknown table type %d", (int)table_type);
    if (num_masks <= 0)
        return set_error(GWBP_EINVAL, "num_masks must be positive (got %d)", (int)num_masks);
    if (D < 4 || D % 4 != 0)
        return set_error(GWBP_EINVAL, "gwbp_scatter_mask_features: D must be a positive multiple of 4 (got %d)", (int)D);
    if ((rc = check_label_map(labels, ls_y, ls_x)))
        return rc;
    if ((rc = check_index_maps("gwbp_scatter_mask_features", ymap, xmap)))
        return rc;
    const uintptr_t talign = table_type == GWBP_MAP_F32 ? 15 : 7; // one float4 / four halves per lane load
    if (!table || ts_row < D || (ts_row & 3) || (reinterpret_cast<uintptr_t>(table) & talign))
        return set_error(GWBP_EINVAL, "table rows must be %d-B aligned runs of D contiguous elements (row stride %lld)",
                         (int)talign + 1, (long long)ts_row);
    if (!F || (reinterpret_cast<uintptr_t>(F) & 15))
        return set_error(GWBP_EINVAL, "F must be a non-null, 16-B aligned [N, D] array");
    if (!slots || (reinterpret_cast<uintptr_t>(slots) & 15))
        return set_error(GWBP_EINVAL, "slots must be a non-null, 16-B aligned buffer");
    // the slot store is sized by the caps alone: checked against the layout before the workspace is bound
    Bound B;
    if ((rc = make_layout(caps, &B.L)))
        return rc;
    if (slots_bytes / GWBP_MASK_SLOT_BYTES < (size_t)B.L.isect_cap)
        return set_error(GWBP_EINVAL, "slots: have %zu bytes, need %d x isect_cap = %zu", slots_bytes, GWBP_MASK_SLOT_BYTES,
                         (size_t)GWBP_MASK_SLOT_BYTES * (size_t)B.L.isect_cap);
    if ((rc = bind(caps, workspace, workspace_bytes, view_host, stream, &B)))
        return rc;
    MaskSlots S;
    S.labels = static_cast<int4 *>(slots);
    S.sums = reinterpret_cast<float4 *>(static_cast<char *>(slots) + (size_t)B.L.isect_cap * sizeof(int4));
    return launch_mask_features(B.L, B.W, B.V, labels, label_type, ls_y, ls_x, ymap, xmap, table, table_type, ts_row, num_masks, D,
                                scale_f, scale_d, F, d, S, n_spilled, B.s);
}

int gwbp_vote_labels(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                     const void *labels, int32_t label_type, int64_t ls_y, int64_t ls_x, const int32_t *ymap, const int32_t *xmap,
                     int32_t num_classes, uint32_t *seen, float *C, int64_t ldc, float *n, void *stream)
{
    // the label, count and bitset arguments before the caps, the workspace or the view
    int rc = check_label_args("gwbp_vote_labels", labels, label_type, ls_y, ls_x, ymap, xmap, num_classes, "C", C, "ldc", ldc);
    if (rc)
        return rc;
    if (!seen || (reinterpret_cast<uintptr_t>(seen) & 3))
        return set_error(GWBP_EINVAL, "seen must be a non-null, 4-B aligned uint32 bitset");
    Bound B;
    if ((rc = bind(caps, workspace, workspace_bytes, view_host, stream, &B)))
        return rc;
    return launch_vote_labels(B.L, B.W, B.V, labels, label_type, ls_y, ls_x, ymap, xmap, num_classes, seen, C, ldc, n, B.s);
}

int gwbp_vote_projected(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                        const void *labels, int32_t label_type, int64_t ls_y, int64_t ls_x, const int32_t *ymap,
                        const int32_t *xmap, const gwbp_pixel_weights *pixel_weights, int32_t num_classes, float *C, int64_t ldc,
                        float *n, void *stream)
{
    PixW P;
    const PixW *pw;
    int rc = check_pixel_weights(pixel_weights, &P, &pw);
    if (rc)
        return rc;
    if ((rc = check_label_args("gwbp_vote_projected", labels, label_type, ls_y, ls_x, ymap, xmap, num_classes, "C", C, "ldc", ldc)))
        return rc;
    Bound B;
    if ((rc = bind(caps, workspace, workspace_bytes, view_host, stream, &B)))
        return rc;
    return launch_vote_projected(B.L, B.W, B.V, labels, label_type, ls_y, ls_x, ymap, xmap, pw, num_classes, C, ldc, n, B.s);
}

int gwbp_label_overlap(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                       const void *labels, int32_t label_type, int64_t ls_y, int64_t ls_x, int32_t num_labels, const int32_t *ymap,
                       const int32_t *xmap, const int32_t *group, int32_t n_cols, int64_t *O, int64_t ldo, void *stream)
{
    Bound B;
    int rc = bind(caps, workspace, workspace_bytes, view_host, stream, &B);
    if (rc)
        return rc;
    if ((rc = check_assoc_args("gwbp_label_overlap", labels, label_type, ls_y, ls_x, ymap, xmap, num_labels, "group", group, n_cols,
                               "O", O, "ldo", ldo)))
        return rc;
    return launch_label_overlap(B.L, B.W, B.V, labels, label_type, ls_y, ls_x, ymap, xmap, num_labels, group, n_cols, O, ldo, B.s);
}

int gwbp_label_votes(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host, const void *labels,
                     int32_t label_type, int64_t ls_y, int64_t ls_x, int32_t num_labels, const int32_t *ymap, const int32_t *xmap,
                     const int32_t *remap, int32_t n_cols, int64_t *V, int64_t ldv, void *stream)
{
    Bound B;
    int rc = bind(caps, workspace, workspace_bytes, view_host, stream, &B);
    if (rc)
        return rc;
    if ((rc = check_assoc_args("gwbp_label_votes", labels, label_type, ls_y, ls_x, ymap, xmap, num_labels, "remap", remap, n_cols,
                               "V", V, "ldv", ldv)))
        return rc;
    return launch_label_votes(B.L, B.W, B.V, labels, label_type, ls_y, ls_x, ymap, xmap, num_labels, remap, n_cols, V, ldv, B.s);
}

int gwbp_label_votes_sparse(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                            const void *labels, int32_t label_type, int64_t ls_y, int64_t ls_x, int32_t num_labels, const int32_t *ymap,
                            const int32_t *xmap, const int32_t *remap, int32_t slots, int32_t *keys, int64_t ld_keys, int64_t *vals,
                            int64_t ld_vals, int64_t *spill, int64_t *total, void *stream)
{
    Bound B;
    int rc = bind(caps, workspace, workspace_bytes, view_host, stream, &B);
    if (rc)
        return rc;
    if ((rc = check_label_type(label_type)))
        return rc;
    if (num_labels <= 0)
        return set_error(GWBP_EINVAL, "num_labels must be positive (got %d)", (int)num_labels);
    if (!remap)
        return set_error(GWBP_EINVAL, "null remap");
    if ((rc = check_sparse_lists(B.L.n, slots, keys, ld_keys, vals, ld_vals, spill, total)))
        return rc;
    if ((rc = check_index_maps("gwbp_label_votes_sparse", ymap, xmap)))
        return rc;
    if ((rc = check_label_map(labels, ls_y, ls_x)))
        return rc;
    return launch_label_votes_sparse(B.L, B.W, B.V, labels, label_type, ls_y, ls_x, ymap, xmap, num_labels, remap, slots, keys, ld_keys,
                                     vals, ld_vals, spill, total, B.s);
}

// What the two typed renders add to the untyped functions' checks: the table's row stride and the alignment of the table and of out to
// their elements (an fp32 pointer of the untyped functions was never looked at: a misaligned one is refused here as well).
static int check_render_payload(const char *what, const void *colors, int32_t color_type, int64_t ldc, int32_t D, const void *out,
                                int32_t out_type)
{
    if (ldc < D)
        return set_error(GWBP_EINVAL, "%s: row stride %lld below D = %d", what, (long long)ldc, (int)D);
    if (fp32_off(colors, color_type) || fp32_off(out, out_type))
        return set_error(GWBP_EINVAL, "%s: fp32 colors and out must be 4-B aligned", what);
    if (int rc = check_half_alignment(what, "colors", colors, color_type))
        return rc;
    if (int rc = check_half_alignment(what, "out", out, out_type))
        return rc;
    if (out_type != GWBP_MAP_F32 && colors == static_cast<const void *>(out))
        return set_error(GWBP_EINVAL, "%s: a half out must not alias colors", what);
    return GWBP_OK;
}

int gwbp_render_typed(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host, const void *colors,
                      int32_t color_type, int64_t ldc, int32_t D, void *out, int32_t out_type, void *stream)
{
    if (int rc = check_field_type("render (color_type)", color_type))
        return rc;
    if (int rc = check_field_type("render (out_type)", out_type))
        return rc;
    Bound B;
    int rc = bind(caps, workspace, workspace_bytes, view_host, stream, &B);
    if (rc)
        return rc;
    if (!colors || !out || D < 1)
        return set_error(GWBP_EINVAL, "bad render arguments");
    if ((rc = check_render_payload("render", colors, color_type, ldc, D, out, out_type)))
        return rc;
    return launch_render(B.L, B.W, B.V, colors, color_type, ldc, D, out, out_type, B.s);
}

int gwbp_render(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                const float *colors, int32_t D, float *out, void *stream)
{
    return gwbp_render_typed(caps, workspace, workspace_bytes, view_host, colors, GWBP_MAP_F32, D, D, out, GWBP_MAP_F32, stream);
}

int gwbp_render_pixels_typed(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                             const void *colors, int32_t color_type, int64_t ldc, int32_t D, float *out, float *alphas, void *stream)
{
    if (int rc = check_field_type("render_pixels", color_type))
        return rc;
    Bound B;
    int rc = bind(caps, workspace, workspace_bytes, view_host, stream, &B);
    if (rc)
        return rc;
    if (!colors || !out || D < 1 || D > 32)
        return set_error(GWBP_EINVAL, "render_pixels needs colors, out and 1 <= D <= 32 (got D=%d)", D);
    if ((rc = check_render_payload("render_pixels", colors, color_type, ldc, D, out, GWBP_MAP_F32)))
        return rc;
    if (reinterpret_cast<uintptr_t>(alphas) & 3)
        return set_error(GWBP_EINVAL, "render_pixels: alphas must be 4-B aligned");
    return launch_render_px(B.W, B.V, colors, color_type, ldc, D, out, alphas, B.s);
}

int gwbp_render_pixels(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                       const float *colors, int32_t D, float *out, float *alphas, void *stream)
{
    return gwbp_render_pixels_typed(caps, workspace, workspace_bytes, view_host, colors, GWBP_MAP_F32, D, D, out, alphas, stream);
}

int gwbp_render_pixels_backward(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                                const float *colors, int64_t ldc, int32_t D, const float *v_out, const float *v_alpha, float *v_colors,
                                float *v_g2d, void *stream)
{
    Bound B;
    int rc = bind(caps, workspace, workspace_bytes, view_host, stream, &B);
    if (rc)
        return rc;
    if (D < 1 || D > 32)
        return set_error(GWBP_EINVAL, "render_pixels_backward needs 1 <= D <= 32 (got D=%d)", D);
    if (!colors || !v_out || !v_g2d)
        return set_error(GWBP_EINVAL, "render_pixels_backward needs colors, v_out and v_g2d (got %s colors, %s v_out, %s v_g2d)",
                         colors ? "a" : "null", v_out ? "a" : "null", v_g2d ? "a" : "null");
    if ((rc = check_render_payload("render_pixels_backward", colors, GWBP_MAP_F32, ldc, D, v_out, GWBP_MAP_F32)))
        return rc;
    if ((reinterpret_cast<uintptr_t>(v_alpha) | reinterpret_cast<uintptr_t>(v_colors) | reinterpret_cast<uintptr_t>(v_g2d)) & 3)
        return set_error(GWBP_EINVAL, "render_pixels_backward: v_alpha, v_colors and v_g2d must be 4-B aligned");
    return launch_render_px_bwd(B.W, B.V, colors, ldc, D, v_out, v_alpha, v_colors, v_g2d, B.s);
}

int gwbp_render_dots_backward(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                              const float *colors, int64_t ldc, int32_t D, const float *v_out, const float *v_alpha, float *v_g2d,
                              void *stream)
{
    Bound B;
    int rc = bind(caps, workspace, workspace_bytes, view_host, stream, &B);
    if (rc)
        return rc;
    if (D < 1 || D > 128)
        return set_error(GWBP_EINVAL, "render_dots_backward needs 1 <= D <= 128 (got D=%d)", D);
    if (!colors || !v_out || !v_g2d)
        return set_error(GWBP_EINVAL, "render_dots_backward needs colors, v_out and v_g2d (got %s colors, %s v_out, %s v_g2d)",
                         colors ? "a" : "null", v_out ? "a" : "null", v_g2d ? "a" : "null");
    if ((rc = check_render_payload("render_dots_backward", colors, GWBP_MAP_F32, ldc, D, v_out, GWBP_MAP_F32)))
        return rc;
    if ((reinterpret_cast<uintptr_t>(v_alpha) | reinterpret_cast<uintptr_t>(v_g2d)) & 3)
        return set_error(GWBP_EINVAL, "render_dots_backward: v_alpha and v_g2d must be 4-B aligned");
    return launch_render_dots_bwd(B.W, B.V, colors, ldc, D, v_out, v_alpha, v_g2d, B.s);
}

int gwbp_project_backward_blocks(int64_t n_gaussians)
{
    if (n_gaussians < 0 || (n_gaussians + kScanBlock - 1) / kScanBlock > 0x7FFFFFFF)
        return set_error(GWBP_EINVAL, "project_backward_blocks: %lld Gaussians out of range", (long long)n_gaussians);
    return project_backward_blocks(n_gaussians);
}

int gwbp_project_backward(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                          int32_t camera_model, int32_t rasterize_mode, const float *means, const float *quats, const float *scales,
                          const float *opacities, const float *v_g2d, float *v_means, float *v_quats, float *v_scales,
                          float *v_opacities, double *v_viewmat, double *scratch, void *stream)
{
    Bound B;
    int rc = bind(caps, workspace, workspace_bytes, view_host, stream, &B);
    if (rc)
        return rc;
    if (camera_model != GWBP_CAMERA_PINHOLE && camera_model != GWBP_CAMERA_ORTHO && camera_model != GWBP_CAMERA_FISHEYE)
        return set_error(GWBP_EINVAL, "unknown camera model %d", (int)camera_model);
    if (rasterize_mode != GWBP_RASTERIZE_CLASSIC && rasterize_mode != GWBP_RASTERIZE_ANTIALIASED)
        return set_error(GWBP_EINVAL, "unknown rasterize mode %d", (int)rasterize_mode);
    if (!means || !quats || !scales || !opacities || !v_g2d)
        return set_error(GWBP_EINVAL, "project_backward needs means, quats, scales, opacities and v_g2d (got %s means, %s quats, %s "
                         "scales, %s opacities, %s v_g2d)", means ? "a" : "null", quats ? "a" : "null", scales ? "a" : "null",
                         opacities ? "a" : "null", v_g2d ? "a" : "null");
    if (!v_means && !v_quats && !v_scales && !v_opacities && !v_viewmat)
        return set_error(GWBP_EINVAL, "project_backward: every output is null");
    if (v_viewmat && !scratch)
        return set_error(GWBP_EINVAL, "project_backward: v_viewmat needs the scratch (gwbp_project_backward_blocks(N) x 12 doubles)");
    if ((reinterpret_cast<uintptr_t>(quats) | reinterpret_cast<uintptr_t>(v_quats)) & 15)
        return set_error(GWBP_EINVAL, "project_backward: quats and v_quats must be 16-B aligned");
    if ((reinterpret_cast<uintptr_t>(means) | reinterpret_cast<uintptr_t>(scales) | reinterpret_cast<uintptr_t>(opacities) |
         reinterpret_cast<uintptr_t>(v_g2d) | reinterpret_cast<uintptr_t>(v_means) | reinterpret_cast<uintptr_t>(v_scales) |
         reinterpret_cast<uintptr_t>(v_opacities)) & 3)
        return set_error(GWBP_EINVAL, "project_backward: means, scales, opacities, v_g2d, v_means, v_scales and v_opacities must be "
                         "4-B aligned");
    if ((reinterpret_cast<uintptr_t>(v_viewmat) | reinterpret_cast<uintptr_t>(scratch)) & 7)
        return set_error(GWBP_EINVAL, "project_backward: v_viewmat and scratch must be 8-B aligned");
    return launch_project_bwd(B.L, B.W, B.V, camera_model, rasterize_mode, means, quats, scales, opacities, v_g2d, v_means, v_quats,
                              v_scales, v_opacities, v_viewmat, scratch, B.s);
}

int gwbp_sh_colors(int64_t N, int32_t degree, int32_t K, const float *means, const float *coeffs,
                   const float *campos_host, float *out, void *stream)
{
    if (N < 0 || degree < 0 || degree > 3 || K < (degree + 1) * (degree + 1) || !campos_host ||
        (N > 0 && (!means || !coeffs || !out)))
        return set_error(GWBP_EINVAL, "bad sh_colors arguments (N=%lld degree=%d K=%d)", (long long)N, degree, K);
    return launch_sh_colors(N, degree, K, means, coeffs, campos_host, out, as_stream(stream));
}

int gwbp_backproject_view(const gwbp_caps *caps, void *workspace, size_t workspace_bytes,
                          const gwbp_view *view_host, const float *means, const float *quats, const float *scales,
                          const float *opacities, const float *feats, int64_t fs_y, int64_t fs_x, int64_t fs_c,
                          int32_t D, float scale_f, float scale_d, float *F, float *d, void *stream)
{
    Bound B;
    int rc = bind(caps, workspace, workspace_bytes, view_host, stream, &B);
    if (rc)
        return rc;
    if ((rc = check_feats(feats, fs_y, fs_x, fs_c, D)))
        return rc;
    if (!F && B.L.n > 0)
        return set_error(GWBP_EINVAL, "null F");
    if (B.L.n > 0 && (!means || !quats || !scales || !opacities))
        return set_error(GWBP_EINVAL, "null Gaussian parameter pointer");
    if (reinterpret_cast<uintptr_t>(quats) & 15)
        return set_error(GWBP_EINVAL, "quats must be 16-B aligned");
    if ((rc = launch_project(B.L, B.W, B.V, means, quats, scales, opacities, nullptr, nullptr, nullptr, nullptr, B.s)))
        return rc;
    if ((rc = launch_bin_sort(B.L, B.W, B.V, nullptr, nullptr, nullptr, B.s)))
        return rc;
    if ((rc = launch_blend(B.L, B.W, B.V, nullptr, nullptr, 0.f, B.s)))
        return rc;
    const FeatMap M{feats, fs_y, fs_x, fs_c, nullptr, nullptr, nullptr, nullptr, 0, 0};
    return launch_scatter(B.L, B.W, B.V, M, D, scale_f, scale_d, F, d, B.s);
}

int gwbp_encode_map(const float *feats, int64_t fs_y, int64_t fs_x, int32_t height, int32_t width, int32_t K,
                    const float *encoder, int32_t n_out, float *out, int32_t workgroups, void *stream)
{
    if (!feats || !encoder || !out || height < 1 || width < 1 || K < 16 || K % 16 != 0 || K > 2048 || n_out < 1 ||
        n_out > 16 || fs_y < 0 || fs_x < 0)
        return set_error(GWBP_EINVAL, "bad encode_map arguments (%dx%d K=%d n_out=%d): K %% 16 == 0, K <= 2048, n_out <= 16",
                         height, width, K, n_out);
    if ((reinterpret_cast<uintptr_t>(feats) & 15) || (fs_y & 3) || (fs_x & 3))
        return set_error(GWBP_EINVAL, "encode_map needs channel-contiguous pixels at 16-B aligned addresses");
    return launch_encode_map(feats, fs_y, fs_x, height, width, K, encoder, n_out, out, workgroups < 0 ? 0 : workgroups,
                             as_stream(stream));
}

int gwbp_finalize_typed(int64_t N, int32_t D, const float *F, const float *d, void *out, int32_t out_type, void *stream)
{
    if (int rc = check_field_type("finalize", out_type))
        return rc;
    if (N < 0 || D < 1 || (N > 0 && (!F || !d || !out)))
        return set_error(GWBP_EINVAL, "bad finalize arguments");
    if (fp32_off(out, out_type))
        return set_error(GWBP_EINVAL, "finalize: out must be 4-B aligned");
    if (int rc = check_half_alignment("finalize", "out", out, out_type))
        return rc;
    if (out_type != GWBP_MAP_F32 && out == static_cast<const void *>(F))
        return set_error(GWBP_EINVAL, "finalize: a half out cannot alias F");
    return launch_finalize(N, D, F, d, out, out_type, as_stream(stream));
}

int gwbp_finalize(int64_t N, int32_t D, const float *F, const float *d, float *out, void *stream)
{
    return gwbp_finalize_typed(N, D, F, d, out, GWBP_MAP_F32, stream);
}

int gwbp_knn_search_typed(int64_t N, int32_t M, int32_t D, int32_t k, const void *Q, int32_t field_type, int64_t ldq, const float *S,
                          int64_t lds_, int32_t *idx, float *score, void *stream)
{
    if (int rc = check_field_type("knn_search", field_type))
        return rc;
    if (N < 0 || M < 1 || D < 1)
        return set_error(GWBP_EINVAL, "knn_search: bad sizes (N=%lld M=%d D=%d)", (long long)N, (int)M, (int)D);
    if (k < 1 || k > 32)
        return set_error(GWBP_EINVAL, "knn_search: k must be in [1, 32] (got %d)", (int)k);
    if (k > M)
        return set_error(GWBP_EINVAL, "knn_search: k = %d exceeds the number of sources M = %d", (int)k, (int)M);
    if (ldq < D || lds_ < D)
        return set_error(GWBP_EINVAL, "knn_search: row strides (%lld, %lld) below D = %d", (long long)ldq, (long long)lds_, (int)D);
    if (!S || (N > 0 && (!Q || !idx || !score)))
        return set_error(GWBP_EINVAL, "knn_search: null Q, S, idx or score");
    if (fp32_off(Q, field_type) || (reinterpret_cast<uintptr_t>(S) & 3))
        return set_error(GWBP_EINVAL, "knn_search: Q and S must be 4-B aligned");
    if (int rc = check_half_alignment("knn_search", "Q", Q, field_type))
        return rc;
    return launch_knn_search(N, M, D, k, Q, field_type, ldq, S, lds_, idx, score, as_stream(stream));
}

int gwbp_knn_search(int64_t N, int32_t M, int32_t D, int32_t k, const float *Q, int64_t ldq, const float *S, int64_t lds_,
                    int32_t *idx, float *score, void *stream)
{
    return gwbp_knn_search_typed(N, M, D, k, Q, GWBP_MAP_F32, ldq, S, lds_, idx, score, stream);
}

int gwbp_knn_vote(int64_t N, int32_t M, int32_t k, const int32_t *idx, const int32_t *labels, int32_t num_classes,
                  int32_t *label_out, int32_t *counts, int64_t ldc, void *stream)
{
    if (N < 0 || M < 1)
        return set_error(GWBP_EINVAL, "knn_vote: bad sizes (N=%lld M=%d)", (long long)N, (int)M);
    if (k < 1 || k > 32)
        return set_error(GWBP_EINVAL, "knn_vote: k must be in [1, 32] (got %d)", (int)k);
    if (num_classes <= 0)
        return set_error(GWBP_EINVAL, "knn_vote: num_classes must be positive (got %d)", (int)num_classes);
    if (counts && ldc < num_classes)
        return set_error(GWBP_EINVAL, "knn_vote: ldc %lld < num_classes %d", (long long)ldc, (int)num_classes);
    if (!labels || (N > 0 && (!idx || !label_out)))
        return set_error(GWBP_EINVAL, "knn_vote: null idx, labels or label_out");
    return launch_knn_vote(N, M, k, idx, labels, num_classes, label_out, counts, ldc, as_stream(stream));
}

// the grid of the spatial entry points: finite lo, a positive finite cell edge, 1 .. 1024 cells per axis, 2^24 in all
static int check_spatial_grid(const char *what, float lo_x, float lo_y, float lo_z, float h, int32_t nx, int32_t ny, int32_t nz)
{
    if (!(fabsf(lo_x) < INFINITY && fabsf(lo_y) < INFINITY && fabsf(lo_z) < INFINITY))
        return set_error(GWBP_EINVAL, "%s: the grid's origin must be finite", what);
    if (!(h >= GWBP_SPATIAL_MIN_CELL && h < INFINITY))
        return set_error(GWBP_EINVAL, "%s: cell size must be finite and at least %g (got %g)", what, (double)GWBP_SPATIAL_MIN_CELL,
                         (double)h);
    if (nx < 1 || ny < 1 || nz < 1 || nx > GWBP_SPATIAL_MAX_DIM || ny > GWBP_SPATIAL_MAX_DIM || nz > GWBP_SPATIAL_MAX_DIM ||
        (int64_t)nx * ny * nz > GWBP_SPATIAL_MAX_CELLS)
        return set_error(GWBP_EINVAL, "%s: grid dimensions %d x %d x %d outside [1, %d] per axis, %d cells in all", what, (int)nx,
                         (int)ny, (int)nz, GWBP_SPATIAL_MAX_DIM, GWBP_SPATIAL_MAX_CELLS);
    return GWBP_OK;
}

static int check_spatial_points(const char *what, const char *name, int64_t n, const float *P, int64_t ldp)
{
    if (n < 0 || n > 0x7FFFFFFF)
        return set_error(GWBP_EINVAL, "%s: bad number of %s (%lld): 0 .. 2^31 - 1", what, name, (long long)n);
    if (ldp < 3)
        return set_error(GWBP_EINVAL, "%s: row stride %lld of %s below 3", what, (long long)ldp, name);
    if (n > 0 && !P)
        return set_error(GWBP_EINVAL, "%s: null %s", what, name);
    if (reinterpret_cast<uintptr_t>(P) & 3)
        return set_error(GWBP_EINVAL, "%s: %s must be 4-B aligned", what, name);
    return GWBP_OK;
}

int gwbp_spatial_cell_keys(int64_t n, const float *points, int64_t ldp, float lo_x, float lo_y, float lo_z, float cell_size,
                           int32_t nx, int32_t ny, int32_t nz, int32_t *keys, void *stream)
{
    if (int rc = check_spatial_points("spatial_cell_keys", "points", n, points, ldp))
        return rc;
    if (int rc = check_spatial_grid("spatial_cell_keys", lo_x, lo_y, lo_z, cell_size, nx, ny, nz))
        return rc;
    if (n > 0 && !keys)
        return set_error(GWBP_EINVAL, "spatial_cell_keys: null keys");
    const float lo[3] = {lo_x, lo_y, lo_z};
    const int32_t dims[3] = {nx, ny, nz};
    return launch_spatial_cell_keys(n, points, ldp, lo, cell_size, dims, keys, as_stream(stream));
}

int gwbp_spatial_build(int64_t n, const float *points, int64_t ldp, const int32_t *sorted_keys, const int64_t *perm,
                       int64_t n_cells, float *sorted, int32_t *cell_start, void *stream)
{
    if (int rc = check_spatial_points("spatial_build", "points", n, points, ldp))
        return rc;
    if (n_cells < 1 || n_cells > GWBP_SPATIAL_MAX_CELLS)
        return set_error(GWBP_EINVAL, "spatial_build: n_cells = %lld outside [1, %d]", (long long)n_cells, GWBP_SPATIAL_MAX_CELLS);
    if (!cell_start || (n > 0 && (!sorted_keys || !perm || !sorted)))
        return set_error(GWBP_EINVAL, "spatial_build: null sorted_keys, perm, sorted or cell_start");
    if (reinterpret_cast<uintptr_t>(sorted) & 15)
        return set_error(GWBP_EINVAL, "spatial_build: sorted must be 16-B aligned");
    return launch_spatial_build(n, points, ldp, sorted_keys, perm, n_cells, sorted, cell_start, as_stream(stream));
}

int gwbp_spatial_knn(int64_t n, const float *sorted, const int32_t *cell_start, float lo_x, float lo_y, float lo_z, float cell_size,
                     int32_t nx, int32_t ny, int32_t nz, int64_t q, const float *queries, int64_t ldq, const int64_t *order,
                     int32_t k, int32_t *idx, float *dist, void *stream)
{
    if (n < 1 || n > 0x7FFFFFFF)
        return set_error(GWBP_EINVAL, "spatial_knn: bad number of points (%lld): 1 .. 2^31 - 1", (long long)n);
    if (k < 1 || k > 32)
        return set_error(GWBP_EINVAL, "spatial_knn: k must be in [1, 32] (got %d)", (int)k);
    if (k > n)
        return set_error(GWBP_EINVAL, "spatial_knn: k = %d exceeds the number of points N = %lld", (int)k, (long long)n);
    if (int rc = check_spatial_points("spatial_knn", "queries", q, queries, ldq))
        return rc;
    if (int rc = check_spatial_grid("spatial_knn", lo_x, lo_y, lo_z, cell_size, nx, ny, nz))
        return rc;
    if (!sorted || !cell_start || (q > 0 && (!order || !idx || !dist)))
        return set_error(GWBP_EINVAL, "spatial_knn: null sorted, cell_start, order, idx or dist");
    if (reinterpret_cast<uintptr_t>(sorted) & 15)
        return set_error(GWBP_EINVAL, "spatial_knn: sorted must be 16-B aligned");
    const float lo[3] = {lo_x, lo_y, lo_z};
    const int32_t dims[3] = {nx, ny, nz};
    return launch_spatial_knn(sorted, cell_start, lo, cell_size, dims, q, queries, ldq, order, k, idx, dist, as_stream(stream));
}

int gwbp_neighbor_mean_out_typed(int64_t n, int64_t m, int32_t D, int32_t k, const int32_t *idx, const void *features,
                                 int32_t field_type, int64_t ldf, void *out, int32_t out_type, int64_t ldo, void *stream)
{
    if (int rc = check_field_type("neighbor_mean", field_type))
        return rc;
    if (int rc = check_field_type("neighbor_mean (out_type)", out_type))
        return rc;
    if (n < 0 || m < 1 || m > 0x7FFFFFFF || D < 1)
        return set_error(GWBP_EINVAL, "neighbor_mean: bad sizes (n=%lld m=%lld D=%d)", (long long)n, (long long)m, (int)D);
    if (k < 1 || k > 32)
        return set_error(GWBP_EINVAL, "neighbor_mean: k must be in [1, 32] (got %d)", (int)k);
    if (ldf < D || ldo < D)
        return set_error(GWBP_EINVAL, "neighbor_mean: row strides (%lld, %lld) below D = %d", (long long)ldf, (long long)ldo, (int)D);
    if (!features || (n > 0 && (!idx || !out)))
        return set_error(GWBP_EINVAL, "neighbor_mean: null idx, features or out");
    if (fp32_off(features, field_type) || fp32_off(out, out_type))
        return set_error(GWBP_EINVAL, "neighbor_mean: features and out must be 4-B aligned");
    if (int rc = check_half_alignment("neighbor_mean", "features", features, field_type))
        return rc;
    if (int rc = check_half_alignment("neighbor_mean", "out", out, out_type))
        return rc;
    if (features == static_cast<const void *>(out))
        return set_error(GWBP_EINVAL, "neighbor_mean: out must not be the features (no alias, whatever its type)");
    return launch_neighbor_mean(n, m, D, k, idx, features, field_type, ldf, out, out_type, ldo, as_stream(stream));
}

int gwbp_neighbor_mean_typed(int64_t n, int64_t m, int32_t D, int32_t k, const int32_t *idx, const void *features, int32_t field_type,
                             int64_t ldf, float *out, int64_t ldo, void *stream)
{
    return gwbp_neighbor_mean_out_typed(n, m, D, k, idx, features, field_type, ldf, out, GWBP_MAP_F32, ldo, stream);
}

int gwbp_neighbor_mean(int64_t n, int64_t m, int32_t D, int32_t k, const int32_t *idx, const float *features, int64_t ldf,
                       float *out, int64_t ldo, void *stream)
{
    return gwbp_neighbor_mean_typed(n, m, D, k, idx, features, GWBP_MAP_F32, ldf, out, ldo, stream);
}

// what the three walks of the radius components share: the built grid of n points, r2 and (when not null) aligned int32 arrays
static int check_radius_walk(const char *what, int64_t n, const float *sorted, const int32_t *cell_start, float lo_x, float lo_y,
                             float lo_z, float h, int32_t nx, int32_t ny, int32_t nz, const int32_t *group, float r2)
{
    if (n < 1 || n > 0x7FFFFFFF)
        return set_error(GWBP_EINVAL, "%s: bad number of points (%lld): 1 .. 2^31 - 1", what, (long long)n);
    if (!(r2 >= 0.0f))
        return set_error(GWBP_EINVAL, "%s: r2 must be >= 0 (got %g)", what, (double)r2);
    if (int rc = check_spatial_grid(what, lo_x, lo_y, lo_z, h, nx, ny, nz))
        return rc;
    if (!sorted || !cell_start)
        return set_error(GWBP_EINVAL, "%s: null sorted or cell_start", what);
    if (reinterpret_cast<uintptr_t>(sorted) & 15)
        return set_error(GWBP_EINVAL, "%s: sorted must be 16-B aligned", what);
    if ((reinterpret_cast<uintptr_t>(cell_start) & 3) || (reinterpret_cast<uintptr_t>(group) & 3))
        return set_error(GWBP_EINVAL, "%s: cell_start and group must be 4-B aligned", what);
    return GWBP_OK;
}

int gwbp_radius_count(int64_t n, const float *sorted, const int32_t *cell_start, float lo_x, float lo_y, float lo_z, float cell_size,
                      int32_t nx, int32_t ny, int32_t nz, const int32_t *group, float r2, int64_t q, const float *queries,
                      int64_t ldq, const int64_t *order, const int32_t *query_group, int32_t cap, int32_t *count, int32_t *visited,
                      void *stream)
{
    if (int rc = check_radius_walk("radius_count", n, sorted, cell_start, lo_x, lo_y, lo_z, cell_size, nx, ny, nz, group, r2))
        return rc;
    if (cap < 1)
        return set_error(GWBP_EINVAL, "radius_count: cap must be at least 1 (got %d)", (int)cap);
    if (int rc = check_spatial_points("radius_count", "queries", q, queries, ldq))
        return rc;
    if (q > 0 && (!order || !count))
        return set_error(GWBP_EINVAL, "radius_count: null order or count");
    if ((reinterpret_cast<uintptr_t>(order) & 7) || (reinterpret_cast<uintptr_t>(query_group) & 3) ||
        (reinterpret_cast<uintptr_t>(count) & 3) || (reinterpret_cast<uintptr_t>(visited) & 3))
        return set_error(GWBP_EINVAL, "radius_count: order must be 8-B aligned, query_group, count and visited 4-B");
    const float lo[3] = {lo_x, lo_y, lo_z};
    const int32_t dims[3] = {nx, ny, nz};
    return launch_radius_count(sorted, cell_start, lo, cell_size, dims, group, r2, q, queries, ldq, order, query_group, cap, count,
                               visited, as_stream(stream));
}

int gwbp_radius_union(int64_t n, const float *sorted, const int32_t *cell_start, float lo_x, float lo_y, float lo_z, float cell_size,
                      int32_t nx, int32_t ny, int32_t nz, const int32_t *group, float r2, const int32_t *count, int32_t min_points,
                      int32_t *parent, int32_t *status, void *stream)
{
    if (int rc = check_radius_walk("radius_union", n, sorted, cell_start, lo_x, lo_y, lo_z, cell_size, nx, ny, nz, group, r2))
        return rc;
    if (min_points < 1)
        return set_error(GWBP_EINVAL, "radius_union: min_points must be at least 1 (got %d)", (int)min_points);
    if (!count || !parent || !status)
        return set_error(GWBP_EINVAL, "radius_union: null count, parent or status");
    if ((reinterpret_cast<uintptr_t>(count) & 3) || (reinterpret_cast<uintptr_t>(parent) & 3) || (reinterpret_cast<uintptr_t>(status) & 3))
        return set_error(GWBP_EINVAL, "radius_union: count, parent and status must be 4-B aligned");
    const float lo[3] = {lo_x, lo_y, lo_z};
    const int32_t dims[3] = {nx, ny, nz};
    return launch_radius_union(n, sorted, cell_start, lo, cell_size, dims, group, r2, count, min_points, parent, status,
                               as_stream(stream));
}

int gwbp_radius_attach(int64_t n, const float *sorted, const int32_t *cell_start, float lo_x, float lo_y, float lo_z, float cell_size,
                       int32_t nx, int32_t ny, int32_t nz, const int32_t *group, float r2, const int32_t *count, int32_t min_points,
                       int32_t *attach, void *stream)
{
    if (int rc = check_radius_walk("radius_attach", n, sorted, cell_start, lo_x, lo_y, lo_z, cell_size, nx, ny, nz, group, r2))
        return rc;
    if (min_points < 1)
        return set_error(GWBP_EINVAL, "radius_attach: min_points must be at least 1 (got %d)", (int)min_points);
    if (!count || !attach)
        return set_error(GWBP_EINVAL, "radius_attach: null count or attach");
    if ((reinterpret_cast<uintptr_t>(count) & 3) || (reinterpret_cast<uintptr_t>(attach) & 3))
        return set_error(GWBP_EINVAL, "radius_attach: count and attach must be 4-B aligned");
    const float lo[3] = {lo_x, lo_y, lo_z};
    const int32_t dims[3] = {nx, ny, nz};
    return launch_radius_attach(n, sorted, cell_start, lo, cell_size, dims, group, r2, count, min_points, attach, as_stream(stream));
}

int gwbp_components_flatten(int64_t n, const int32_t *count, int32_t min_points, const int32_t *attach, int32_t *parent,
                            int32_t *root, int32_t *status, void *stream)
{
    if (n < 1 || n > 0x7FFFFFFF)
        return set_error(GWBP_EINVAL, "components_flatten: bad number of points (%lld): 1 .. 2^31 - 1", (long long)n);
    if (min_points < 1)
        return set_error(GWBP_EINVAL, "components_flatten: min_points must be at least 1 (got %d)", (int)min_points);
    if (!count || !parent || !root || !status)
        return set_error(GWBP_EINVAL, "components_flatten: null count, parent, root or status");
    if ((reinterpret_cast<uintptr_t>(count) & 3) || (reinterpret_cast<uintptr_t>(attach) & 3) || (reinterpret_cast<uintptr_t>(parent) & 3) ||
        (reinterpret_cast<uintptr_t>(root) & 3) || (reinterpret_cast<uintptr_t>(status) & 3))
        return set_error(GWBP_EINVAL, "components_flatten: count, attach, parent, root and status must be 4-B aligned");
    if (root == parent)
        return set_error(GWBP_EINVAL, "components_flatten: root must not be parent");
    return launch_components_flatten(n, count, min_points, attach, parent, root, status, as_stream(stream));
}

// an array a region entry point writes must be none of the arrays it reads, and no two written arrays the same
static int check_regions_distinct(const char *what, const void *const *written, int n_written, const void *const *read, int n_read)
{
    for (int a = 0; a < n_written; ++a) {
        for (int b = a + 1; b < n_written; ++b)
            if (written[a] == written[b])
                return set_error(GWBP_EINVAL, "%s: two output arrays are the same array", what);
        for (int b = 0; b < n_read; ++b)
            if (read[b] && written[a] == read[b])
                return set_error(GWBP_EINVAL, "%s: an output array must not be one of the input arrays", what);
    }
    return GWBP_OK;
}

// what the two region entry points share: the neighbour list idx[n, k] and the similarities of its entries
static int check_neighbor_list(const char *what, int64_t n, int32_t k, const int32_t *idx, const float *sim)
{
    if (n < 1 || n > 0x7FFFFFFF)
        return set_error(GWBP_EINVAL, "%s: bad number of rows (%lld): 1 .. 2^31 - 1", what, (long long)n);
    if (k < 1 || k > GWBP_REGIONS_MAX_K)
        return set_error(GWBP_EINVAL, "%s: k must be in [1, %d] (got %d)", what, GWBP_REGIONS_MAX_K, (int)k);
    if (!idx || !sim)
        return set_error(GWBP_EINVAL, "%s: null idx or sim", what);
    if ((reinterpret_cast<uintptr_t>(idx) & 3) || (reinterpret_cast<uintptr_t>(sim) & 3))
        return set_error(GWBP_EINVAL, "%s: idx and sim must be 4-B aligned", what);
    return GWBP_OK;
}

int gwbp_neighbor_similarity_typed(int64_t n, int32_t D, int32_t k, const int32_t *idx, const void *features, int32_t field_type,
                                   int64_t ldf, float *sim, int32_t *live, void *stream)
{
    if (int rc = check_field_type("neighbor_similarity", field_type))
        return rc;
    if (int rc = check_neighbor_list("neighbor_similarity", n, k, idx, sim))
        return rc;
    if (D < 1 || D > GWBP_REGIONS_MAX_D)
        return set_error(GWBP_EINVAL, "neighbor_similarity: D must be in [1, %d] (got %d)", GWBP_REGIONS_MAX_D, (int)D);
    if (ldf < D)
        return set_error(GWBP_EINVAL, "neighbor_similarity: row stride %lld below D = %d", (long long)ldf, (int)D);
    if (!features || !live)
        return set_error(GWBP_EINVAL, "neighbor_similarity: null features or live");
    if (fp32_off(features, field_type) || (reinterpret_cast<uintptr_t>(live) & 3))
        return set_error(GWBP_EINVAL, "neighbor_similarity: features and live must be 4-B aligned");
    if (int rc = check_half_alignment("neighbor_similarity", "features", features, field_type))
        return rc;
    const void *const written[] = {sim, live}, *const read[] = {idx, features};
    if (int rc = check_regions_distinct("neighbor_similarity", written, 2, read, 2))
        return rc;
    return launch_neighbor_similarity(n, D, k, idx, features, field_type, ldf, sim, live, as_stream(stream));
}

int gwbp_neighbor_similarity(int64_t n, int32_t D, int32_t k, const int32_t *idx, const float *features, int64_t ldf, float *sim,
                             int32_t *live, void *stream)
{
    return gwbp_neighbor_similarity_typed(n, D, k, idx, features, GWBP_MAP_F32, ldf, sim, live, stream);
}

int gwbp_edge_union(int64_t n, int32_t k, const int32_t *idx, const float *sim, const int32_t *live, const float *dist,
                    const int32_t *group, float sim_min, float max_dist, int32_t *count, int32_t *parent, int32_t *status,
                    void *stream)
{
    if (int rc = check_neighbor_list("edge_union", n, k, idx, sim))
        return rc;
    if (sim_min != sim_min)
        return set_error(GWBP_EINVAL, "edge_union: sim_min must not be NaN");
    if (!(max_dist >= 0.0f))
        return set_error(GWBP_EINVAL, "edge_union: max_dist must be >= 0 or +inf (got %g)", (double)max_dist);
    if (!live || !count || !parent || !status)
        return set_error(GWBP_EINVAL, "edge_union: null live, count, parent or status");
    if ((reinterpret_cast<uintptr_t>(live) & 3) || (reinterpret_cast<uintptr_t>(dist) & 3) || (reinterpret_cast<uintptr_t>(group) & 3) ||
        (reinterpret_cast<uintptr_t>(count) & 3) || (reinterpret_cast<uintptr_t>(parent) & 3) || (reinterpret_cast<uintptr_t>(status) & 3))
        return set_error(GWBP_EINVAL, "edge_union: live, dist, group, count, parent and status must be 4-B aligned");
    const void *const written[] = {count, parent, status}, *const read[] = {idx, sim, live, dist, group};
    if (int rc = check_regions_distinct("edge_union", written, 3, read, 5))
        return rc;
    return launch_edge_union(n, k, idx, sim, live, dist, group, sim_min, max_dist, count, parent, status, as_stream(stream));
}

// ---- point samples (sample.hip) ----------------------------------------------------------------------------------------------------
static bool misaligned(const void *p, unsigned mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

// a neighbour list with weights: idx[q, k] and w[q, k], dense
static int check_weighted_list(const char *what, int64_t q, int64_t m, int32_t k, const int32_t *idx, const float *w)
{
    if (q < 0 || q > 0x7FFFFFFF || m < 1 || m > 0x7FFFFFFF)
        return set_error(GWBP_EINVAL, "%s: bad sizes (q=%lld m=%lld): 0 <= q < 2^31, 1 <= m < 2^31", what, (long long)q, (long long)m);
    if (k < 1 || k > GWBP_SAMPLE_MAX_K)
        return set_error(GWBP_EINVAL, "%s: k must be in [1, %d] (got %d)", what, GWBP_SAMPLE_MAX_K, (int)k);
    if (q > 0 && (!idx || !w))
        return set_error(GWBP_EINVAL, "%s: null idx or w", what);
    if (misaligned(idx, 3) || misaligned(w, 3))
        return set_error(GWBP_EINVAL, "%s: idx and w must be 4-B aligned", what);
    return GWBP_OK;
}

int gwbp_gaussian_pack(int64_t n, const float *means, int64_t ldm, const float *quats, int64_t ldq, const float *scales, int64_t lds_,
                       const float *opacities, const uint8_t *live, const int64_t *perm, float *pack, void *stream)
{
    if (n < 1 || n > 0x7FFFFFFF)
        return set_error(GWBP_EINVAL, "gaussian_pack: bad number of Gaussians (%lld): 1 .. 2^31 - 1", (long long)n);
    if (ldm < 3 || ldq < 4 || lds_ < 3)
        return set_error(GWBP_EINVAL, "gaussian_pack: row strides (%lld, %lld, %lld) of means, quats, scales below (3, 4, 3)",
                         (long long)ldm, (long long)ldq, (long long)lds_);
    if (!means || !quats || !scales || !opacities || !perm || !pack)
        return set_error(GWBP_EINVAL, "gaussian_pack: null means, quats, scales, opacities, perm or pack");
    if (misaligned(means, 3) || misaligned(quats, 3) || misaligned(scales, 3) || misaligned(opacities, 3) || misaligned(perm, 7) ||
        misaligned(pack, 15))
        return set_error(GWBP_EINVAL, "gaussian_pack: means, quats, scales and opacities must be 4-B aligned, perm 8-B, pack 16-B");
    const void *const written[] = {pack}, *const read[] = {means, quats, scales, opacities, live, perm};
    if (int rc = check_regions_distinct("gaussian_pack", written, 1, read, 6))
        return rc;
    return launch_gaussian_pack(n, means, ldm, quats, ldq, scales, lds_, opacities, live, perm, pack, as_stream(stream));
}

int gwbp_point_gaussians(int64_t n, const float *sorted, const int32_t *cell_start, float lo_x, float lo_y, float lo_z, float cell_size,
                         int32_t nx, int32_t ny, int32_t nz, const float *pack, float r2, float alpha_min, int64_t q,
                         const float *queries, int64_t ldq, const int64_t *order, int32_t k, int32_t *idx, float *w, int32_t *n_contrib,
                         int32_t *visited, void *stream)
{
    if (int rc = check_radius_walk("point_gaussians", n, sorted, cell_start, lo_x, lo_y, lo_z, cell_size, nx, ny, nz, nullptr, r2))
        return rc;
    if (k < 1 || k > GWBP_SAMPLE_MAX_K)
        return set_error(GWBP_EINVAL, "point_gaussians: k must be in [1, %d] (got %d)", GWBP_SAMPLE_MAX_K, (int)k);
    if (!(alpha_min >= GWBP_SAMPLE_MIN_ALPHA && alpha_min <= 1.0f))
        return set_error(GWBP_EINVAL, "point_gaussians: alpha_min must be in [%g, 1] (got %g)", (double)GWBP_SAMPLE_MIN_ALPHA,
                         (double)alpha_min);
    if (int rc = check_spatial_points("point_gaussians", "queries", q, queries, ldq))
        return rc;
    if (!pack || (q > 0 && (!order || !idx || !w || !n_contrib)))
        return set_error(GWBP_EINVAL, "point_gaussians: null pack, order, idx, w or n_contrib");
    if (misaligned(pack, 15) || misaligned(order, 7) || misaligned(idx, 3) || misaligned(w, 3) || misaligned(n_contrib, 3) ||
        misaligned(visited, 3))
        return set_error(GWBP_EINVAL, "point_gaussians: pack must be 16-B aligned, order 8-B, idx, w, n_contrib and visited 4-B");
    const void *const written[] = {idx, w, n_contrib, visited}, *const read[] = {sorted, cell_start, pack, queries, order};
    if (q > 0)
        if (int rc = check_regions_distinct("point_gaussians", written, visited ? 4 : 3, read, 5))
            return rc;
    const float lo[3] = {lo_x, lo_y, lo_z};
    const int32_t dims[3] = {nx, ny, nz};
    return launch_point_gaussians(sorted, cell_start, lo, cell_size, dims, pack, r2, alpha_min, q, queries, ldq, order, k, idx, w,
                                  n_contrib, visited, as_stream(stream));
}

int gwbp_neighbor_blend_out_typed(int64_t q, int64_t m, int32_t D, int32_t k, const int32_t *idx, const float *w, const void *features,
                                  int32_t field_type, int64_t ldf, void *out, int32_t out_type, int64_t ldo, float *wsum, void *stream)
{
    if (int rc = check_field_type("neighbor_blend", field_type))
        return rc;
    if (int rc = check_field_type("neighbor_blend (out_type)", out_type))
        return rc;
    if (int rc = check_weighted_list("neighbor_blend", q, m, k, idx, w))
        return rc;
    if (D < 1)
        return set_error(GWBP_EINVAL, "neighbor_blend: D must be at least 1 (got %d)", (int)D);
    if (ldf < D || ldo < D)
        return set_error(GWBP_EINVAL, "neighbor_blend: row strides (%lld, %lld) below D = %d", (long long)ldf, (long long)ldo, (int)D);
    if (!features || (q > 0 && (!out || !wsum)))
        return set_error(GWBP_EINVAL, "neighbor_blend: null features, out or wsum");
    if (fp32_off(features, field_type) || fp32_off(out, out_type) || misaligned(wsum, 3))
        return set_error(GWBP_EINVAL, "neighbor_blend: features, out and wsum must be 4-B aligned");
    if (int rc = check_half_alignment("neighbor_blend", "features", features, field_type))
        return rc;
    if (int rc = check_half_alignment("neighbor_blend", "out", out, out_type))
        return rc;
    const void *const written[] = {out, wsum}, *const read[] = {idx, w, features};
    if (q > 0)
        if (int rc = check_regions_distinct("neighbor_blend", written, 2, read, 3))
            return rc;
    return launch_neighbor_blend(q, m, D, k, idx, w, features, field_type, ldf, out, out_type, ldo, wsum, as_stream(stream));
}

int gwbp_neighbor_blend_typed(int64_t q, int64_t m, int32_t D, int32_t k, const int32_t *idx, const float *w, const void *features,
                              int32_t field_type, int64_t ldf, float *out, int64_t ldo, float *wsum, void *stream)
{
    return gwbp_neighbor_blend_out_typed(q, m, D, k, idx, w, features, field_type, ldf, out, GWBP_MAP_F32, ldo, wsum, stream);
}

int gwbp_neighbor_blend(int64_t q, int64_t m, int32_t D, int32_t k, const int32_t *idx, const float *w, const float *features,
                        int64_t ldf, float *out, int64_t ldo, float *wsum, void *stream)
{
    return gwbp_neighbor_blend_typed(q, m, D, k, idx, w, features, GWBP_MAP_F32, ldf, out, ldo, wsum, stream);
}

int gwbp_weighted_vote(int64_t q, int64_t m, int32_t k, const int32_t *idx, const float *w, const int32_t *labels, int32_t num_classes,
                       int32_t *out_label, float *out_share, void *stream)
{
    if (int rc = check_weighted_list("weighted_vote", q, m, k, idx, w))
        return rc;
    if (num_classes < 1)
        return set_error(GWBP_EINVAL, "weighted_vote: num_classes must be at least 1 (got %d)", (int)num_classes);
    if (!labels || (q > 0 && (!out_label || !out_share)))
        return set_error(GWBP_EINVAL, "weighted_vote: null labels, out_label or out_share");
    if (misaligned(labels, 3) || misaligned(out_label, 3) || misaligned(out_share, 3))
        return set_error(GWBP_EINVAL, "weighted_vote: labels, out_label and out_share must be 4-B aligned");
    const void *const written[] = {out_label, out_share}, *const read[] = {idx, w, labels};
    if (q > 0)
        if (int rc = check_regions_distinct("weighted_vote", written, 2, read, 3))
            return rc;
    return launch_weighted_vote(q, m, k, idx, w, labels, num_classes, out_label, out_share, as_stream(stream));
}

// the checks the two passes of the fit share
static int check_pca_rows(const char *what, int64_t N, int32_t D, const void *X, int32_t field_type, int64_t ldx, const void *workspace,
                          size_t workspace_bytes)
{
    if (int rc = check_field_type(what, field_type))
        return rc;
    if (N < 2 || D < 1 || D > GWBP_PCA_MAX_D)
        return set_error(GWBP_EINVAL, "%s: bad sizes (N=%lld D=%d): N >= 2, 1 <= D <= %d", what, (long long)N, (int)D,
                         GWBP_PCA_MAX_D);
    if (ldx < D)
        return set_error(GWBP_EINVAL, "%s: row stride %lld below D = %d", what, (long long)ldx, (int)D);
    if (!X || !workspace)
        return set_error(GWBP_EINVAL, "%s: null X or workspace", what);
    if (fp32_off(X, field_type) || (reinterpret_cast<uintptr_t>(workspace) & 7))
        return set_error(GWBP_EINVAL, "%s: X must be 4-B aligned, the workspace 8-B", what);
    if (int rc = check_half_alignment(what, "X", X, field_type))
        return rc;
    const size_t need = pca_workspace_bytes(N, D);
    if (workspace_bytes < need)
        return set_error(GWBP_EWORKSPACE, "%s: workspace has %zu bytes, needs %zu", what, workspace_bytes, need);
    return GWBP_OK;
}

int gwbp_pca_workspace_size(int64_t N, int32_t D, size_t *bytes)
{
    if (N < 2 || D < 1 || D > GWBP_PCA_MAX_D || !bytes)
        return set_error(GWBP_EINVAL, "pca_workspace_size: bad arguments (N=%lld D=%d): N >= 2, 1 <= D <= %d", (long long)N, (int)D,
                         GWBP_PCA_MAX_D);
    *bytes = pca_workspace_bytes(N, D);
    return GWBP_OK;
}

int gwbp_column_means_typed(int64_t N, int32_t D, const void *X, int32_t field_type, int64_t ldx, float *mean_out, void *workspace,
                            size_t workspace_bytes, void *stream)
{
    const int rc = check_pca_rows("column_means", N, D, X, field_type, ldx, workspace, workspace_bytes);
    if (rc)
        return rc;
    if (!mean_out)
        return set_error(GWBP_EINVAL, "column_means: null mean_out");
    return launch_column_means(N, D, X, field_type, ldx, mean_out, workspace, as_stream(stream));
}

int gwbp_column_means(int64_t N, int32_t D, const float *X, int64_t ldx, float *mean_out, void *workspace, size_t workspace_bytes,
                      void *stream)
{
    return gwbp_column_means_typed(N, D, X, GWBP_MAP_F32, ldx, mean_out, workspace, workspace_bytes, stream);
}

int gwbp_centered_gram_typed(int64_t N, int32_t D, const void *X, int32_t field_type, int64_t ldx, const float *mean, double *gram_out,
                             void *workspace, size_t workspace_bytes, void *stream)
{
    const int rc = check_pca_rows("centered_gram", N, D, X, field_type, ldx, workspace, workspace_bytes);
    if (rc)
        return rc;
    if (!mean || !gram_out || (reinterpret_cast<uintptr_t>(gram_out) & 7))
        return set_error(GWBP_EINVAL, "centered_gram: null mean or gram_out, or gram_out not 8-B aligned");
    return launch_centered_gram(N, D, X, field_type, ldx, mean, gram_out, workspace, as_stream(stream));
}

int gwbp_centered_gram(int64_t N, int32_t D, const float *X, int64_t ldx, const float *mean, double *gram_out, void *workspace,
                       size_t workspace_bytes, void *stream)
{
    return gwbp_centered_gram_typed(N, D, X, GWBP_MAP_F32, ldx, mean, gram_out, workspace, workspace_bytes, stream);
}

int gwbp_pca_project_typed(int64_t N, int32_t D, int32_t k, const void *X, int32_t field_type, int64_t ldx, const float *mean,
                           const float *components, float *Y, float *minmax_partials, void *stream)
{
    if (int rc = check_field_type("pca_project", field_type))
        return rc;
    if (N < 1 || D < 1 || D > GWBP_PCA_MAX_D)
        return set_error(GWBP_EINVAL, "pca_project: bad sizes (N=%lld D=%d): N >= 1, 1 <= D <= %d", (long long)N, (int)D,
                         GWBP_PCA_MAX_D);
    if (k < 1 || k > GWBP_PCA_MAX_K)
        return set_error(GWBP_EINVAL, "pca_project: k must be in [1, %d] (got %d)", GWBP_PCA_MAX_K, (int)k);
    if (ldx < D)
        return set_error(GWBP_EINVAL, "pca_project: row stride %lld below D = %d", (long long)ldx, (int)D);
    if (!X || !mean || !components || !Y || !minmax_partials)
        return set_error(GWBP_EINVAL, "pca_project: null X, mean, components, Y or minmax_partials");
    if (fp32_off(X, field_type))
        return set_error(GWBP_EINVAL, "pca_project: X must be 4-B aligned");
    if (int rc = check_half_alignment("pca_project", "X", X, field_type))
        return rc;
    return launch_pca_project(N, D, k, X, field_type, ldx, mean, components, Y, minmax_partials, as_stream(stream));
}

int gwbp_pca_project(int64_t N, int32_t D, int32_t k, const float *X, int64_t ldx, const float *mean, const float *components,
                     float *Y, float *minmax_partials, void *stream)
{
    return gwbp_pca_project_typed(N, D, k, X, GWBP_MAP_F32, ldx, mean, components, Y, minmax_partials, stream);
}

int gwbp_pca_colors(int64_t n, const float *Y, const float *lo_hi, float *colors, void *stream)
{
    if (n < 0 || !lo_hi || (n > 0 && (!Y || !colors)))
        return set_error(GWBP_EINVAL, "pca_colors: bad arguments");
    return launch_pca_colors(n, Y, lo_hi, colors, as_stream(stream));
}

// What the clustering entry points share: the sizes, and the field's stride and pointer, checked once for all of them.
static int check_cluster_sizes(const char *what, int64_t N, int32_t K, int32_t D)
{
    if (N < 0)
        return set_error(GWBP_EINVAL, "%s: N must not be negative (got %lld)", what, (long long)N);
    if (K < 1 || K > GWBP_CLUSTER_MAX_K)
        return set_error(GWBP_EINVAL, "%s: K must be in [1, %d] (got %d)", what, GWBP_CLUSTER_MAX_K, (int)K);
    if (D < 1)
        return set_error(GWBP_EINVAL, "%s: D must be positive (got %d)", what, (int)D);
    return GWBP_OK;
}

static int check_cluster_rows(const char *what, int64_t N, int32_t K, int32_t D, const void *X, int32_t field_type, int64_t ldx)
{
    if (int rc = check_field_type(what, field_type))
        return rc;
    if (int rc = check_cluster_sizes(what, N, K, D))
        return rc;
    if (ldx < D)
        return set_error(GWBP_EINVAL, "%s: row stride %lld of X below D = %d", what, (long long)ldx, (int)D);
    if (N > 0 && !X)
        return set_error(GWBP_EINVAL, "%s: null X", what);
    if (fp32_off(X, field_type))
        return set_error(GWBP_EINVAL, "%s: X must be 4-B aligned", what);
    return check_half_alignment(what, "X", X, field_type);
}

int gwbp_kmeans_assign_typed(int64_t N, int32_t K, int32_t D, const void *X, int32_t field_type, int64_t ldx, const float *C, int64_t ldc,
                             const float *b, int32_t *label, float *best, void *stream)
{
    if (int rc = check_cluster_rows("kmeans_assign", N, K, D, X, field_type, ldx))
        return rc;
    if (ldc < D)
        return set_error(GWBP_EINVAL, "kmeans_assign: row stride ldc = %lld of C below D = %d", (long long)ldc, (int)D);
    if (!C || (N > 0 && (!label || !best)))
        return set_error(GWBP_EINVAL, "kmeans_assign: null C, label or best");
    if ((reinterpret_cast<uintptr_t>(C) & 3) || (reinterpret_cast<uintptr_t>(b) & 3) || (reinterpret_cast<uintptr_t>(label) & 3) ||
        (reinterpret_cast<uintptr_t>(best) & 3))
        return set_error(GWBP_EINVAL, "kmeans_assign: C, b, label and best must be 4-B aligned");
    return launch_kmeans_assign(N, K, D, X, field_type, ldx, C, ldc, b, label, best, as_stream(stream));
}

int gwbp_kmeans_assign(int64_t N, int32_t K, int32_t D, const float *X, int64_t ldx, const float *C, int64_t ldc, const float *b,
                       int32_t *label, float *best, void *stream)
{
    return gwbp_kmeans_assign_typed(N, K, D, X, GWBP_MAP_F32, ldx, C, ldc, b, label, best, stream);
}

int gwbp_cluster_workspace_size(int64_t N, int32_t D, int32_t K, size_t *bytes)
{
    if (int rc = check_cluster_sizes("cluster_workspace_size", N, K, D))
        return rc;
    if (!bytes)
        return set_error(GWBP_EINVAL, "cluster_workspace_size: null bytes");
    *bytes = cluster_workspace_bytes(N, D, K);
    return GWBP_OK;
}

int gwbp_cluster_sums_typed(int64_t N, int32_t D, int32_t K, const void *X, int32_t field_type, int64_t ldx, const float *w,
                            const int64_t *order, const int64_t *start, double *sums, double *wsum, void *workspace,
                            size_t workspace_bytes, void *stream)
{
    if (int rc = check_cluster_rows("cluster_sums", N, K, D, X, field_type, ldx))
        return rc;
    if (!start || (N > 0 && !order))
        return set_error(GWBP_EINVAL, "cluster_sums: null start or order");
    if (!sums || !wsum || !workspace)
        return set_error(GWBP_EINVAL, "cluster_sums: null sums, wsum or workspace");
    if (reinterpret_cast<uintptr_t>(w) & 3)
        return set_error(GWBP_EINVAL, "cluster_sums: w must be 4-B aligned");
    if ((reinterpret_cast<uintptr_t>(order) & 7) || (reinterpret_cast<uintptr_t>(start) & 7) || (reinterpret_cast<uintptr_t>(sums) & 7) ||
        (reinterpret_cast<uintptr_t>(wsum) & 7) || (reinterpret_cast<uintptr_t>(workspace) & 7))
        return set_error(GWBP_EINVAL, "cluster_sums: order, start, sums, wsum and the workspace must be 8-B aligned");
    const size_t need = cluster_workspace_bytes(N, D, K);
    if (workspace_bytes < need)
        return set_error(GWBP_EWORKSPACE, "cluster_sums: workspace has %zu bytes, needs %zu", workspace_bytes, need);
    return launch_cluster_sums(N, D, K, X, field_type, ldx, w, order, start, sums, wsum, workspace, as_stream(stream));
}

int gwbp_cluster_sums(int64_t N, int32_t D, int32_t K, const float *X, int64_t ldx, const float *w, const int64_t *order,
                      const int64_t *start, double *sums, double *wsum, void *workspace, size_t workspace_bytes, void *stream)
{
    return gwbp_cluster_sums_typed(N, D, K, X, GWBP_MAP_F32, ldx, w, order, start, sums, wsum, workspace, workspace_bytes, stream);
}

// The field as the two queries read it: D, the row stride and the pointer, checked once for both.
static int check_field_rows(const char *what, int32_t D, const void *X, int64_t ldx, int32_t field_type = GWBP_MAP_F32)
{
    if (D < 1 || D > GWBP_PCA_MAX_D)
        return set_error(GWBP_EINVAL, "%s: D must be in [1, %d] (got %d)", what, GWBP_PCA_MAX_D, (int)D);
    if (ldx < D)
        return set_error(GWBP_EINVAL, "%s: row stride %lld below D = %d", what, (long long)ldx, (int)D);
    if (!X)
        return set_error(GWBP_EINVAL, "%s: null X", what);
    if (fp32_off(X, field_type))
        return set_error(GWBP_EINVAL, "%s: X must be 4-B aligned", what);
    return check_half_alignment(what, "X", X, field_type);
}

int gwbp_prompt_scores_typed(int64_t N, int32_t D, int32_t P, int32_t n_pos, const void *X, int32_t field_type, int64_t ldx,
                             const float *prompts, int32_t normalize, const float *threshold_host, uint8_t *mask, float *scores,
                             void *stream)
{
    if (int rc = check_field_type("prompt_scores", field_type))
        return rc;
    if (N < 0)
        return set_error(GWBP_EINVAL, "prompt_scores: N must not be negative (got %lld)", (long long)N);
    if (P < 1 || P > GWBP_QUERY_MAX_P)
        return set_error(GWBP_EINVAL, "prompt_scores: P must be in [1, %d] (got %d)", GWBP_QUERY_MAX_P, (int)P);
    if (n_pos < 1 || n_pos > P)
        return set_error(GWBP_EINVAL, "prompt_scores: n_pos must be in [1, P = %d] (got %d)", (int)P, (int)n_pos);
    const int rc = check_field_rows("prompt_scores", D, X, ldx, field_type);
    if (rc)
        return rc;
    if (!prompts || (reinterpret_cast<uintptr_t>(prompts) & 3))
        return set_error(GWBP_EINVAL, "prompt_scores: prompts must be a non-null, 4-B aligned [P, D] array");
    if (!mask && !scores)
        return set_error(GWBP_EINVAL, "prompt_scores: mask and scores are both null");
    if (reinterpret_cast<uintptr_t>(scores) & 3)
        return set_error(GWBP_EINVAL, "prompt_scores: scores must be 4-B aligned");
    if (mask && n_pos == P && !threshold_host)
        return set_error(GWBP_EINVAL, "prompt_scores: a mask without negative prompts (n_pos == P) needs a threshold");
    return launch_prompt_scores(N, D, P, n_pos, X, field_type, ldx, prompts, normalize != 0, threshold_host, mask, scores,
                                as_stream(stream));
}

int gwbp_prompt_scores(int64_t N, int32_t D, int32_t P, int32_t n_pos, const float *X, int64_t ldx, const float *prompts,
                       int32_t normalize, const float *threshold_host, uint8_t *mask, float *scores, void *stream)
{
    return gwbp_prompt_scores_typed(N, D, P, n_pos, X, GWBP_MAP_F32, ldx, prompts, normalize, threshold_host, mask, scores, stream);
}

int gwbp_probe_pixels_typed(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host, int32_t M,
                            const int32_t *xy, const void *X, int32_t field_type, int64_t ldx, int32_t D, float *out, float *depth,
                            float *alpha, void *stream)
{
    if (int rc0 = check_field_type("probe_pixels", field_type))
        return rc0;
    // the probe's own arguments first: nothing of the caps, the workspace or the view is looked at before they pass
    if (M < 1 || M > GWBP_PROBE_MAX_PIXELS)
        return set_error(GWBP_EINVAL, "probe_pixels: M must be in [1, %d] (got %d)", GWBP_PROBE_MAX_PIXELS, (int)M);
    int rc = check_field_rows("probe_pixels", D, X, ldx, field_type);
    if (rc)
        return rc;
    if (!xy || !out || (reinterpret_cast<uintptr_t>(xy) & 3) || (reinterpret_cast<uintptr_t>(out) & 3))
        return set_error(GWBP_EINVAL, "probe_pixels: xy and out must be non-null and 4-B aligned");
    if ((reinterpret_cast<uintptr_t>(depth) & 3) || (reinterpret_cast<uintptr_t>(alpha) & 3))
        return set_error(GWBP_EINVAL, "probe_pixels: depth and alpha must be 4-B aligned");
    Bound B;
    if ((rc = bind(caps, workspace, workspace_bytes, view_host, stream, &B)))
        return rc;
    return launch_probe_pixels(B.W, B.V, M, xy, X, field_type, ldx, D, out, depth, alpha, B.s);
}

int gwbp_probe_pixels(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host, int32_t M,
                      const int32_t *xy, const float *X, int64_t ldx, int32_t D, float *out, float *depth, float *alpha,
                      void *stream)
{
    return gwbp_probe_pixels_typed(caps, workspace, workspace_bytes, view_host, M, xy, X, GWBP_MAP_F32, ldx, D, out, depth, alpha, stream);
}

int gwbp_pixel_gaussians(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host, int32_t k, int32_t M,
                         const int32_t *xy, int32_t *ids, float *weights, int32_t *n_contrib, float *alpha, int32_t *median_id,
                         float *median_depth, void *stream)
{
    // the call's own arguments first: nothing of the caps, the workspace or the view is looked at before they pass
    if (k < 1 || k > GWBP_PIXEL_TOPK_MAX)
        return set_error(GWBP_EINVAL, "pixel_gaussians: k must be in [1, %d] (got %d)", GWBP_PIXEL_TOPK_MAX, (int)k);
    if (xy && (M < 1 || M > GWBP_PROBE_MAX_PIXELS))
        return set_error(GWBP_EINVAL, "pixel_gaussians: M must be in [1, %d] (got %d)", GWBP_PROBE_MAX_PIXELS, (int)M);
    if (reinterpret_cast<uintptr_t>(xy) & 3)
        return set_error(GWBP_EINVAL, "pixel_gaussians: xy must be 4-B aligned");
    if (!ids || !weights || (reinterpret_cast<uintptr_t>(ids) & 3) || (reinterpret_cast<uintptr_t>(weights) & 3))
        return set_error(GWBP_EINVAL, "pixel_gaussians: ids and weights must be non-null and 4-B aligned");
    if ((reinterpret_cast<uintptr_t>(n_contrib) & 3) || (reinterpret_cast<uintptr_t>(alpha) & 3) ||
        (reinterpret_cast<uintptr_t>(median_id) & 3) || (reinterpret_cast<uintptr_t>(median_depth) & 3))
        return set_error(GWBP_EINVAL, "pixel_gaussians: n_contrib, alpha, median_id and median_depth must be 4-B aligned");
    Bound B;
    if (int rc = bind(caps, workspace, workspace_bytes, view_host, stream, &B))
        return rc;
    return launch_pixel_gaussians(B.W, B.V, k, M, xy, ids, weights, n_contrib, alpha, median_id, median_depth, B.s);
}

int gwbp_render_labels(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                       const int32_t *labels, int32_t num_classes, float *maps, float *alphas, int32_t *argmax, float *argmax_sums,
                       float min_opacity, const int32_t *gt, int32_t cut, uint64_t *counts, void *stream)
{
    // the call's own arguments first: nothing of the caps, the workspace or the view is looked at before they pass
    if (num_classes < 1 || num_classes > GWBP_RENDER_LABELS_MAX_CLASSES)
        return set_error(GWBP_EINVAL, "render_labels: num_classes must be in [1, %d] (got %d)", GWBP_RENDER_LABELS_MAX_CLASSES,
                         (int)num_classes);
    if (!labels || (reinterpret_cast<uintptr_t>(labels) & 3))
        return set_error(GWBP_EINVAL, "render_labels: labels must be a non-null, 4-B aligned int32 [N] array");
    if (!maps && !alphas && !argmax && !argmax_sums && !counts)
        return set_error(GWBP_EINVAL, "render_labels: every output is null");
    if ((reinterpret_cast<uintptr_t>(maps) & 3) || (reinterpret_cast<uintptr_t>(alphas) & 3) ||
        (reinterpret_cast<uintptr_t>(argmax) & 3) || (reinterpret_cast<uintptr_t>(argmax_sums) & 3))
        return set_error(GWBP_EINVAL, "render_labels: maps, alphas, argmax and argmax_sums must be 4-B aligned");
    if (argmax && !argmax_sums && num_classes > 64)
        return set_error(GWBP_EINVAL, "render_labels: argmax of %d > 64 classes needs argmax_sums (the carry between class chunks)",
                         (int)num_classes);
    if (!gt != !counts)
        return set_error(GWBP_EINVAL, "render_labels: gt and counts go together (got %s gt, %s counts)", gt ? "a" : "null",
                         counts ? "a" : "null");
    if ((reinterpret_cast<uintptr_t>(gt) & 3) || (reinterpret_cast<uintptr_t>(counts) & 7))
        return set_error(GWBP_EINVAL, "render_labels: gt must be 4-B aligned, counts 8-B");
    if (cut < 0 || cut > 255)
        return set_error(GWBP_EINVAL, "render_labels: cut must be in [0, 255] (got %d)", (int)cut);
    Bound B;
    const int rc = bind(caps, workspace, workspace_bytes, view_host, stream, &B);
    if (rc)
        return rc;
    return launch_render_labels(B.W, B.V, labels, num_classes, maps, alphas, argmax, argmax_sums, min_opacity, gt, cut,
                                reinterpret_cast<u64 *>(counts), B.s);
}

int gwbp_field_compare_typed(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                             const void *features, int32_t field_type, int64_t ldf, int32_t D, const void *map, int32_t map_type,
                             int64_t ms_y, int64_t ms_x, int32_t lr_h, int32_t lr_w, const int32_t *ymap, const int32_t *xmap,
                             float *planes, double *table, void *stream)
{
    if (int rc0 = check_field_type("field_compare", field_type))
        return rc0;
    // the caps, the workspace and the view first (as gwbp_render), then the call's own arguments, each kind once
    Bound B;
    int rc = bind(caps, workspace, workspace_bytes, view_host, stream, &B);
    if (rc)
        return rc;
    if (!known_map_type(map_type))
        return set_error(GWBP_EINVAL, "field_compare: unknown map type %d", (int)map_type);
    if (D < 1 || D > GWBP_PCA_MAX_D)
        return set_error(GWBP_EINVAL, "field_compare: D must be in [1, %d] (got %d)", GWBP_PCA_MAX_D, (int)D);
    if (ldf < D)
        return set_error(GWBP_EINVAL, "field_compare: row stride %lld below D = %d", (long long)ldf, (int)D);
    if ((!features && B.L.n > 0) || fp32_off(features, field_type))
        return set_error(GWBP_EINVAL, "field_compare: features must be a non-null, 4-B aligned [N, D] array");
    if ((rc = check_half_alignment("field_compare", "features", features, field_type)))
        return rc;
    if (!map || (reinterpret_cast<uintptr_t>(map) & (map_type == GWBP_MAP_F32 ? 3 : 1)))
        return set_error(GWBP_EINVAL, "field_compare: the map must be non-null and aligned to its element type");
    if (ms_y < 0 || ms_x < 0)
        return set_error(GWBP_EINVAL, "field_compare: negative map strides (%lld %lld)", (long long)ms_y, (long long)ms_x);
    if ((rc = check_index_maps("gwbp_field_compare", ymap, xmap)))
        return rc;
    if (ymap && (lr_h < 1 || lr_w < 1))
        return set_error(GWBP_EINVAL, "field_compare: index maps need the low-resolution map's shape (got %d x %d)", (int)lr_h,
                         (int)lr_w);
    if ((reinterpret_cast<uintptr_t>(ymap) & 3) || (reinterpret_cast<uintptr_t>(xmap) & 3))
        return set_error(GWBP_EINVAL, "field_compare: the index maps must be 4-B aligned");
    if (reinterpret_cast<uintptr_t>(planes) & 3)
        return set_error(GWBP_EINVAL, "field_compare: planes must be 4-B aligned");
    if (!table || (reinterpret_cast<uintptr_t>(table) & 7))
        return set_error(GWBP_EINVAL, "field_compare: table must be a non-null, 8-B aligned float64 [8] array");
    if (B.V.tile_w * B.V.tile_h > GWBP_FIELD_COMPARE_MAX_TILES)
        return set_error(GWBP_EINVAL, "field_compare: a view of %d tiles exceeds GWBP_FIELD_COMPARE_MAX_TILES = %d",
                         B.V.tile_w * B.V.tile_h, GWBP_FIELD_COMPARE_MAX_TILES);
    return launch_field_compare(B.L, B.W, B.V, features, field_type, ldf, D, map, map_type, ms_y, ms_x, ymap ? lr_h : 0, ymap ? lr_w : 0,
                                ymap, xmap, planes, table, B.s);
}

int gwbp_field_compare(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                       const float *features, int64_t ldf, int32_t D, const void *map, int32_t map_type, int64_t ms_y, int64_t ms_x,
                       int32_t lr_h, int32_t lr_w, const int32_t *ymap, const int32_t *xmap, float *planes, double *table,
                       void *stream)
{
    return gwbp_field_compare_typed(caps, workspace, workspace_bytes, view_host, features, GWBP_MAP_F32, ldf, D, map, map_type, ms_y,
                                    ms_x, lr_h, lr_w, ymap, xmap, planes, table, stream);
}

// the shape contract of the decode-loss kernels: what they are not built for is unsupported, not invalid
static int check_decode_shape(const char *what, int32_t d, int32_t D)
{
    if (d < 16 || d > 128 || d % 16)
        return set_error(GWBP_EUNSUPPORTED, "%s: d must be a multiple of 16 in [16, 128] (got %d)", what, (int)d);
    if (D < 16 || D > GWBP_PCA_MAX_D || D % 16)
        return set_error(GWBP_EUNSUPPORTED, "%s: D must be a multiple of 16 in [16, %d] (got %d)", what, GWBP_PCA_MAX_D, (int)D);
    return GWBP_OK;
}

int gwbp_decode_loss_workspace_size(int32_t d, int32_t D, size_t *bytes)
{
    const int rc = check_decode_shape("decode_loss_workspace_size", d, D);
    if (rc)
        return rc;
    if (!bytes)
        return set_error(GWBP_EINVAL, "decode_loss_workspace_size: null bytes");
    *bytes = decode_loss_workspace_bytes(d, D);
    return GWBP_OK;
}

int gwbp_decode_loss(int32_t height, int32_t width, int32_t d, int32_t D, const float *R, int64_t ldr, const float *C, int64_t ldc,
                     const void *map, int32_t map_type, int64_t ms_y, int64_t ms_x, const gwbp_pixel_weights *pixel_weights,
                     int32_t loss_kind, float scale, float *GR, int64_t ldg, float *GC, int64_t ldgc, double *table, void *workspace,
                     size_t workspace_bytes, void *stream)
{
    // the pixel weights first (as every call that takes them), then the shape contract, then each kind of argument once
    PixW Pw;
    const PixW *pw;
    int rc = check_pixel_weights(pixel_weights, &Pw, &pw);
    if (rc || (rc = check_decode_shape("decode_loss", d, D)))
        return rc;
    if (height < 0 || width < 0)
        return set_error(GWBP_EINVAL, "decode_loss: negative image size %d x %d", (int)width, (int)height);
    const int64_t P = (int64_t)height * width;
    if (P > GWBP_DECODE_MAX_PIXELS)
        return set_error(GWBP_EUNSUPPORTED, "decode_loss: %lld pixels exceed GWBP_DECODE_MAX_PIXELS = %d", (long long)P,
                         GWBP_DECODE_MAX_PIXELS);
    if (!known_map_type(map_type))
        return set_error(GWBP_EINVAL, "decode_loss: unknown map type %d", (int)map_type);
    if (loss_kind != GWBP_LOSS_L1 && loss_kind != GWBP_LOSS_L2)
        return set_error(GWBP_EINVAL, "decode_loss: unknown loss kind %d", (int)loss_kind);
    if (ldr < d || ldg < d || ldc < D || ldgc < D)
        return set_error(GWBP_EINVAL, "decode_loss: row strides (R %lld, GR %lld, C %lld, GC %lld) below d = %d / D = %d",
                         (long long)ldr, (long long)ldg, (long long)ldc, (long long)ldgc, (int)d, (int)D);
    if (ms_y < 0 || ms_x < 0)
        return set_error(GWBP_EINVAL, "decode_loss: negative map strides (%lld %lld)", (long long)ms_y, (long long)ms_x);
    if (!C || !GC || !table || !workspace || (P > 0 && (!R || !map || !GR)))
        return set_error(GWBP_EINVAL, "decode_loss: null R, C, map, GR, GC, table or workspace");
    if ((reinterpret_cast<uintptr_t>(R) & 3) || (reinterpret_cast<uintptr_t>(C) & 3) || (reinterpret_cast<uintptr_t>(GR) & 3) ||
        (reinterpret_cast<uintptr_t>(GC) & 3) || (reinterpret_cast<uintptr_t>(map) & (map_type == GWBP_MAP_F32 ? 3 : 1)))
        return set_error(GWBP_EINVAL, "decode_loss: R, C, GR and GC must be 4-B aligned, the map to its element type");
    if ((reinterpret_cast<uintptr_t>(table) & 7) || (reinterpret_cast<uintptr_t>(workspace) & 7))
        return set_error(GWBP_EINVAL, "decode_loss: table and workspace must be 8-B aligned");
    const size_t need = decode_loss_workspace_bytes(d, D);
    if (workspace_bytes < need)
        return set_error(GWBP_EWORKSPACE, "decode_loss: workspace has %zu bytes, needs %zu", workspace_bytes, need);
    return launch_decode_loss(height, width, d, D, R, ldr, C, ldc, map, map_type, ms_y, ms_x, pw, loss_kind == GWBP_LOSS_L2, scale,
                              GR, ldg, GC, ldgc, table, workspace, as_stream(stream));
}

// the shape contract of the photometric loss; `what` names the entry point
static int check_image_loss_shape(const char *what, int32_t height, int32_t width, int32_t D, int32_t padding)
{
    if (D < 1 || D > GWBP_IMAGE_LOSS_MAX_D)
        return set_error(GWBP_EINVAL, "%s: D must be in [1, %d] (got %d)", what, GWBP_IMAGE_LOSS_MAX_D, (int)D);
    if (padding != GWBP_SSIM_VALID && padding != GWBP_SSIM_SAME)
        return set_error(GWBP_EINVAL, "%s: unknown padding %d", what, (int)padding);
    if (height < 1 || width < 1)
        return set_error(GWBP_EINVAL, "%s: an image of %d x %d pixels (width x height)", what, (int)width, (int)height);
    if (padding == GWBP_SSIM_VALID && (height < 11 || width < 11))
        return set_error(GWBP_EINVAL, "%s: valid padding needs width and height >= 11, the window's size (got %d x %d)", what,
                         (int)width, (int)height);
    if ((int64_t)height * width > GWBP_IMAGE_LOSS_MAX_PIXELS)
        return set_error(GWBP_EINVAL, "%s: %lld pixels exceed GWBP_IMAGE_LOSS_MAX_PIXELS = %d", what,
                         (long long)((int64_t)height * width), GWBP_IMAGE_LOSS_MAX_PIXELS);
    return GWBP_OK;
}

int gwbp_image_loss_workspace_size(int32_t height, int32_t width, int32_t D, int32_t want_grad, size_t *bytes)
{
    // (the size does not depend on the padding: the tiles cover the image under both)
    const int rc = check_image_loss_shape("image_loss_workspace_size", height, width, D, GWBP_SSIM_SAME);
    if (rc)
        return rc;
    if (!bytes)
        return set_error(GWBP_EINVAL, "image_loss_workspace_size: null bytes");
    *bytes = image_loss_workspace_bytes(height, width, D, want_grad != 0);
    return GWBP_OK;
}

int gwbp_image_loss(int32_t height, int32_t width, int32_t D, const float *x, int64_t xs, const float *y, int64_t ys,
                    const gwbp_pixel_weights *pixel_weights, int32_t padding, float ssim_lambda, float *map, float *grad, int64_t gs,
                    double *table, void *workspace, size_t workspace_bytes, void *stream)
{
    PixW Pw;
    const PixW *pw;
    int rc = check_pixel_weights(pixel_weights, &Pw, &pw);
    if (rc || (rc = check_image_loss_shape("image_loss", height, width, D, padding)))
        return rc;
    if (xs < D || ys < D || (grad && gs < D))
        return set_error(GWBP_EINVAL, "image_loss: pixel strides (x %lld, y %lld, grad %lld) below D = %d", (long long)xs,
                         (long long)ys, (long long)gs, (int)D);
    if (!x || !y || !table || !workspace)
        return set_error(GWBP_EINVAL, "image_loss: null x, y, table or workspace");
    if ((reinterpret_cast<uintptr_t>(x) & 3) || (reinterpret_cast<uintptr_t>(y) & 3) || (reinterpret_cast<uintptr_t>(map) & 3) ||
        (reinterpret_cast<uintptr_t>(grad) & 3))
        return set_error(GWBP_EINVAL, "image_loss: x, y, map and grad must be 4-B aligned");
    if ((reinterpret_cast<uintptr_t>(table) & 7) || (reinterpret_cast<uintptr_t>(workspace) & 7))
        return set_error(GWBP_EINVAL, "image_loss: table and workspace must be 8-B aligned");
    const size_t need = image_loss_workspace_bytes(height, width, D, grad != nullptr);
    if (workspace_bytes < need)
        return set_error(GWBP_EWORKSPACE, "image_loss: workspace has %zu bytes, needs %zu", workspace_bytes, need);
    return launch_image_loss(height, width, D, x, xs, y, ys, pw, padding == GWBP_SSIM_SAME, ssim_lambda, map, grad, gs, table,
                             workspace, as_stream(stream));
}

// ---- densification (densify.hip) ---------------------------------------------------------------------------------------------------
static int check_densify_count(const char *what, int64_t n)
{
    if (n < 0 || n > 0x7FFFFFFF)
        return set_error(GWBP_EINVAL, "%s: bad number of Gaussians (%lld): 0 .. 2^31 - 1", what, (long long)n);
    return GWBP_OK;
}

// n_out rows out of n parents: each leaves at most two
static int check_densify_out(const char *what, int64_t n, int64_t n_out)
{
    if (int rc = check_densify_count(what, n))
        return rc;
    if (n_out < 0 || n_out > 2 * n)
        return set_error(GWBP_EINVAL, "%s: n_out = %lld disagrees with offsets of %lld parents (0 .. %lld rows)", what, (long long)n_out,
                         (long long)n, (long long)(2 * n));
    return GWBP_OK;
}

int gwbp_densify_accumulate(int64_t n, int32_t n_cameras, const float *v_means2d, const int32_t *radii, float sx, float sy, float *grad2d,
                            float *count, void *stream)
{
    if (int rc = check_densify_count("densify_accumulate", n))
        return rc;
    if (n_cameras < 1)
        return set_error(GWBP_EINVAL, "densify_accumulate: n_cameras must be at least 1 (got %d)", (int)n_cameras);
    if (n > 0 && (!v_means2d || !radii || !grad2d || !count))
        return set_error(GWBP_EINVAL, "densify_accumulate: null v_means2d, radii, grad2d or count");
    if (misaligned(v_means2d, 7) || misaligned(radii, 3) || misaligned(grad2d, 3) || misaligned(count, 3))
        return set_error(GWBP_EINVAL, "densify_accumulate: v_means2d must be 8-B aligned, radii, grad2d and count 4-B");
    if (grad2d && grad2d == count)
        return set_error(GWBP_EINVAL, "densify_accumulate: grad2d and count are the same array");
    return launch_densify_accumulate(n, n_cameras, v_means2d, radii, sx, sy, grad2d, count, as_stream(stream));
}

int gwbp_densify_plan_workspace_size(int64_t n, size_t *bytes)
{
    if (int rc = check_densify_count("densify_plan_workspace_size", n))
        return rc;
    if (!bytes)
        return set_error(GWBP_EINVAL, "densify_plan_workspace_size: null bytes");
    *bytes = densify_plan_workspace_bytes(n);
    return GWBP_OK;
}

int gwbp_densify_plan(int64_t n, const float *grad2d, const float *count, const float *scaling, int64_t lds_, const float *opacity,
                      float t_grad, float t_small, float t_big, float t_opa, float log16, int32_t prune_big, uint8_t *kind,
                      int64_t *offsets, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = check_densify_count("densify_plan", n))
        return rc;
    if (lds_ < 3)
        return set_error(GWBP_EINVAL, "densify_plan: row stride %lld of scaling below 3", (long long)lds_);
    if (!offsets || !workspace || (n > 0 && (!grad2d || !count || !scaling || !opacity || !kind)))
        return set_error(GWBP_EINVAL, "densify_plan: null grad2d, count, scaling, opacity, kind, offsets or workspace");
    if (misaligned(grad2d, 3) || misaligned(count, 3) || misaligned(scaling, 3) || misaligned(opacity, 3))
        return set_error(GWBP_EINVAL, "densify_plan: grad2d, count, scaling and opacity must be 4-B aligned");
    if (misaligned(offsets, 7) || misaligned(workspace, 7))
        return set_error(GWBP_EINVAL, "densify_plan: offsets and workspace must be 8-B aligned");
    const size_t need = densify_plan_workspace_bytes(n);
    if (workspace_bytes < need)
        return set_error(GWBP_EWORKSPACE, "densify_plan: workspace has %zu bytes, needs %zu", workspace_bytes, need);
    const float thresholds[5] = {t_grad, t_small, t_big, t_opa, log16};
    return launch_densify_plan(n, grad2d, count, scaling, lds_, opacity, thresholds, prune_big != 0, kind, offsets, workspace,
                               as_stream(stream));
}

int gwbp_densify_emit(int64_t n, int64_t n_out, const uint8_t *kind, const int64_t *offsets, const float *means, const float *scaling,
                      const float *rotation, const float *opacity, const float *noise, float log16, int32_t *parent, uint8_t *child,
                      float *out_means, float *out_scaling, float *out_rotation, float *out_opacity, void *stream)
{
    if (int rc = check_densify_out("densify_emit", n, n_out))
        return rc;
    if (n > 0 && (!kind || !offsets || !means || !scaling || !rotation || !opacity || !noise))
        return set_error(GWBP_EINVAL, "densify_emit: null kind, offsets, means, scaling, rotation, opacity or noise");
    if (n_out > 0 && (!parent || !child || !out_means || !out_scaling || !out_rotation || !out_opacity))
        return set_error(GWBP_EINVAL, "densify_emit: null parent, child or output table");
    if (misaligned(offsets, 7))
        return set_error(GWBP_EINVAL, "densify_emit: offsets must be 8-B aligned");
    if (misaligned(means, 3) || misaligned(scaling, 3) || misaligned(rotation, 3) || misaligned(opacity, 3) || misaligned(noise, 3) ||
        misaligned(parent, 3) || misaligned(out_means, 3) || misaligned(out_scaling, 3) || misaligned(out_rotation, 3) ||
        misaligned(out_opacity, 3))
        return set_error(GWBP_EINVAL, "densify_emit: the float tables and parent must be 4-B aligned");
    const void *const written[] = {out_means, out_scaling, out_rotation, out_opacity}, *const read[] = {means, scaling, rotation, opacity, noise};
    if (n_out > 0)
        if (int rc = check_regions_distinct("densify_emit", written, 4, read, 5))
            return rc;
    return launch_densify_emit(n, n_out, kind, offsets, means, scaling, rotation, opacity, noise, log16, parent, child, out_means,
                               out_scaling, out_rotation, out_opacity, as_stream(stream));
}

int gwbp_densify_gather(int64_t n, int64_t n_out, int32_t w, const float *table, int64_t ldt, const int32_t *parent, const uint8_t *child,
                        const uint8_t *kind, int32_t mode, float *out, int64_t ldo, void *stream)
{
    if (int rc = check_densify_out("densify_gather", n, n_out))
        return rc;
    if (w < 1 || w > GWBP_DENSIFY_MAX_WIDTH)
        return set_error(GWBP_EINVAL, "densify_gather: w must be in [1, %d] (got %d)", GWBP_DENSIFY_MAX_WIDTH, (int)w);
    if (ldt < w || ldo < w)
        return set_error(GWBP_EINVAL, "densify_gather: row strides (%lld, %lld) below w = %d", (long long)ldt, (long long)ldo, (int)w);
    if (mode != GWBP_DENSIFY_COPY && mode != GWBP_DENSIFY_ZERO_NEW)
        return set_error(GWBP_EINVAL, "densify_gather: unknown mode %d", (int)mode);
    if (n_out > 0 && (!table || !parent || !out || (mode == GWBP_DENSIFY_ZERO_NEW && (!child || !kind))))
        return set_error(GWBP_EINVAL, "densify_gather: null table, parent or out (child or kind under GWBP_DENSIFY_ZERO_NEW)");
    if (misaligned(table, 3) || misaligned(parent, 3) || misaligned(out, 3))
        return set_error(GWBP_EINVAL, "densify_gather: table, parent and out must be 4-B aligned");
    if (out && out == table)
        return set_error(GWBP_EINVAL, "densify_gather: out must not be the table");
    return launch_densify_gather(n, n_out, w, table, ldt, parent, child, kind, mode == GWBP_DENSIFY_ZERO_NEW, out, ldo, as_stream(stream));
}

// ---- the MCMC strategy (mcmc.hip) ----------------------------------------------------------------------------------------------------
static int check_mcmc_counts(const char *what, int64_t n, int64_t m)
{
    if (int rc = check_densify_count(what, n))
        return rc;
    if (m < 0 || m > 0x7FFFFFFF)
        return set_error(GWBP_EINVAL, "%s: bad number of draws (%lld): 0 .. 2^31 - 1", what, (long long)m);
    return GWBP_OK;
}

static int check_mcmc_table(const char *what, int32_t w, int64_t ldt)
{
    if (w < 1 || w > GWBP_DENSIFY_MAX_WIDTH)
        return set_error(GWBP_EINVAL, "%s: w must be in [1, %d] (got %d)", what, GWBP_DENSIFY_MAX_WIDTH, (int)w);
    if (ldt < w)
        return set_error(GWBP_EINVAL, "%s: row stride %lld below w = %d", what, (long long)ldt, (int)w);
    return GWBP_OK;
}

int gwbp_mcmc_plan_workspace_size(int64_t n, size_t *bytes)
{
    if (int rc = check_densify_count("mcmc_plan_workspace_size", n))
        return rc;
    if (!bytes)
        return set_error(GWBP_EINVAL, "mcmc_plan_workspace_size: null bytes");
    *bytes = mcmc_plan_workspace_bytes(n);
    return GWBP_OK;
}

int gwbp_mcmc_plan(int64_t n, const float *opacity, float t_opa, int32_t mode, int64_t *cdf, int64_t *dead_offsets, int32_t *dead_idx,
                   void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = check_densify_count("mcmc_plan", n))
        return rc;
    if (mode != GWBP_MCMC_RELOCATE && mode != GWBP_MCMC_ADD)
        return set_error(GWBP_EINVAL, "mcmc_plan: unknown mode %d", (int)mode);
    if (!cdf || !dead_offsets || !workspace || (n > 0 && (!opacity || !dead_idx)))
        return set_error(GWBP_EINVAL, "mcmc_plan: null opacity, cdf, dead_offsets, dead_idx or workspace");
    if (misaligned(opacity, 3) || misaligned(dead_idx, 3))
        return set_error(GWBP_EINVAL, "mcmc_plan: opacity and dead_idx must be 4-B aligned");
    if (misaligned(cdf, 7) || misaligned(dead_offsets, 7) || misaligned(workspace, 7))
        return set_error(GWBP_EINVAL, "mcmc_plan: cdf, dead_offsets and workspace must be 8-B aligned");
    if (cdf == dead_offsets)
        return set_error(GWBP_EINVAL, "mcmc_plan: cdf and dead_offsets are the same array");
    const size_t need = mcmc_plan_workspace_bytes(n);
    if (workspace_bytes < need)
        return set_error(GWBP_EWORKSPACE, "mcmc_plan: workspace has %zu bytes, needs %zu", workspace_bytes, need);
    return launch_mcmc_plan(n, opacity, t_opa, mode == GWBP_MCMC_ADD, cdf, dead_offsets, dead_idx, workspace, as_stream(stream));
}

int gwbp_mcmc_draw(int64_t n, int64_t m, const int64_t *cdf, const double *u, int32_t *parent, void *stream)
{
    if (int rc = check_mcmc_counts("mcmc_draw", n, m))
        return rc;
    if (m > 0 && (!cdf || !u || !parent))
        return set_error(GWBP_EINVAL, "mcmc_draw: null cdf, u or parent");
    if (misaligned(cdf, 7) || misaligned(u, 7))
        return set_error(GWBP_EINVAL, "mcmc_draw: cdf and u must be 8-B aligned");
    if (misaligned(parent, 3))
        return set_error(GWBP_EINVAL, "mcmc_draw: parent must be 4-B aligned");
    return launch_mcmc_draw(n, m, cdf, u, parent, as_stream(stream));
}

int gwbp_mcmc_update(int64_t n, int64_t m, const int32_t *parent, float min_opacity, float *opacity, float *scaling, int64_t lds_,
                     int32_t *count, void *stream)
{
    if (int rc = check_mcmc_counts("mcmc_update", n, m))
        return rc;
    if (!(min_opacity > 0.0f && min_opacity < 1.0f))
        return set_error(GWBP_EINVAL, "mcmc_update: min_opacity must be in (0, 1) (got %g)", (double)min_opacity);
    if (lds_ < 3)
        return set_error(GWBP_EINVAL, "mcmc_update: row stride %lld of scaling below 3", (long long)lds_);
    if ((n > 0 && (!opacity || !scaling || !count)) || (n > 0 && m > 0 && !parent))
        return set_error(GWBP_EINVAL, "mcmc_update: null parent, opacity, scaling or count");
    if (misaligned(parent, 3) || misaligned(opacity, 3) || misaligned(scaling, 3) || misaligned(count, 3))
        return set_error(GWBP_EINVAL, "mcmc_update: parent, opacity, scaling and count must be 4-B aligned");
    return launch_mcmc_update(n, m, parent, min_opacity, opacity, scaling, lds_, count, as_stream(stream));
}

int gwbp_mcmc_move(int64_t n, int64_t m, int32_t w, const int32_t *parent, const int32_t *dead_idx, float *table, int64_t ldt, void *stream)
{
    if (int rc = check_mcmc_counts("mcmc_move", n, m))
        return rc;
    if (int rc = check_mcmc_table("mcmc_move", w, ldt))
        return rc;
    if (n > 0 && m > 0 && (!parent || !dead_idx || !table))
        return set_error(GWBP_EINVAL, "mcmc_move: null parent, dead_idx or table");
    if (misaligned(parent, 3) || misaligned(dead_idx, 3) || misaligned(table, 3))
        return set_error(GWBP_EINVAL, "mcmc_move: parent, dead_idx and table must be 4-B aligned");
    return launch_mcmc_move(n, m, w, parent, dead_idx, table, ldt, as_stream(stream));
}

int gwbp_mcmc_zero_rows(int64_t n, int32_t w, const int32_t *count, float *table, int64_t ldt, void *stream)
{
    if (int rc = check_densify_count("mcmc_zero_rows", n))
        return rc;
    if (int rc = check_mcmc_table("mcmc_zero_rows", w, ldt))
        return rc;
    if (n > 0 && (!count || !table))
        return set_error(GWBP_EINVAL, "mcmc_zero_rows: null count or table");
    if (misaligned(count, 3) || misaligned(table, 3))
        return set_error(GWBP_EINVAL, "mcmc_zero_rows: count and table must be 4-B aligned");
    return launch_mcmc_zero_rows(n, w, count, table, ldt, as_stream(stream));
}

int gwbp_mcmc_noise(int64_t n, float *means, const float *scaling, const float *rotation, const float *opacity, const float *z, float scaler,
                    void *stream)
{
    if (int rc = check_densify_count("mcmc_noise", n))
        return rc;
    if (n > 0 && (!means || !scaling || !rotation || !opacity || !z))
        return set_error(GWBP_EINVAL, "mcmc_noise: null means, scaling, rotation, opacity or z");
    if (misaligned(means, 3) || misaligned(scaling, 3) || misaligned(rotation, 3) || misaligned(opacity, 3) || misaligned(z, 3))
        return set_error(GWBP_EINVAL, "mcmc_noise: the tables must be 4-B aligned");
    const void *const written[] = {means}, *const read[] = {scaling, rotation, opacity, z};
    if (n > 0)
        if (int rc = check_regions_distinct("mcmc_noise", written, 1, read, 4))
            return rc;
    return launch_mcmc_noise(n, means, scaling, rotation, opacity, z, scaler, as_stream(stream));
}

int gwbp_mcmc_libm(int64_t n, int32_t op, const float *a, const float *b, float *out, void *stream)
{
    if (int rc = check_densify_count("mcmc_libm", n))
        return rc;
    if (op != GWBP_MCMC_LIBM_EXP && op != GWBP_MCMC_LIBM_LOG && op != GWBP_MCMC_LIBM_POW)
        return set_error(GWBP_EINVAL, "mcmc_libm: unknown op %d", (int)op);
    if (n > 0 && (!a || !out || (op == GWBP_MCMC_LIBM_POW && !b)))
        return set_error(GWBP_EINVAL, "mcmc_libm: null a, out (or b under GWBP_MCMC_LIBM_POW)");
    if (misaligned(a, 3) || misaligned(b, 3) || misaligned(out, 3))
        return set_error(GWBP_EINVAL, "mcmc_libm: a, b and out must be 4-B aligned");
    return launch_mcmc_libm(n, op, a, b, out, as_stream(stream));
}

// what gwbp_sh_eval and gwbp_sh_eval_backward share: the degree, the split of the coefficient row and the input arrays
static int check_sh_tables(const char *what, int64_t n, int32_t degree, int32_t k_head, int32_t k_tail, const float *means,
                           const float *head, const float *tail, const float *campos_host)
{
    if (int rc = check_densify_count(what, n))
        return rc;
    if (degree < 0 || degree > 3)
        return set_error(GWBP_EINVAL, "%s: degree must be in [0, 3] (got %d)", what, (int)degree);
    if (k_head < 1 || k_tail < 0)
        return set_error(GWBP_EINVAL, "%s: K_head must be at least 1 and K_tail at least 0 (got %d, %d)", what, (int)k_head, (int)k_tail);
    if ((int64_t)k_head + k_tail < (degree + 1) * (degree + 1))
        return set_error(GWBP_EINVAL, "%s: %d + %d coefficients are fewer than the %d of degree %d", what, (int)k_head, (int)k_tail,
                         (degree + 1) * (degree + 1), (int)degree);
    if ((int64_t)k_head + k_tail > GWBP_SH_MAX_K)
        return set_error(GWBP_EINVAL, "%s: %d + %d coefficients are more than GWBP_SH_MAX_K = %d", what, (int)k_head, (int)k_tail,
                         GWBP_SH_MAX_K);
    if (!tail && k_tail > 0)
        return set_error(GWBP_EINVAL, "%s: null tail with K_tail = %d", what, (int)k_tail);
    if (tail && k_tail == 0)
        return set_error(GWBP_EINVAL, "%s: a tail with K_tail = 0", what);
    if (!campos_host)
        return set_error(GWBP_EINVAL, "%s: null campos_host", what);
    if (n > 0 && (!means || !head))
        return set_error(GWBP_EINVAL, "%s: null means or head", what);
    if (misaligned(means, 3) || misaligned(head, 3) || misaligned(tail, 3))
        return set_error(GWBP_EINVAL, "%s: means, head and tail must be 4-B aligned", what);
    return GWBP_OK;
}

int gwbp_sh_eval(int64_t N, int32_t degree, int32_t K_head, int32_t K_tail, const float *means, const float *head, const float *tail,
                 const float *campos_host, float *out, void *stream)
{
    if (int rc = check_sh_tables("sh_eval", N, degree, K_head, K_tail, means, head, tail, campos_host))
        return rc;
    if (N > 0 && !out)
        return set_error(GWBP_EINVAL, "sh_eval: null out");
    if (misaligned(out, 3))
        return set_error(GWBP_EINVAL, "sh_eval: out must be 4-B aligned");
    const void *const written[] = {out}, *const read[] = {means, head, tail};
    if (N > 0)
        if (int rc = check_regions_distinct("sh_eval", written, 1, read, 3))
            return rc;
    return launch_sh_eval(N, degree, K_head, K_tail, means, head, tail, campos_host, out, as_stream(stream));
}

int gwbp_sh_eval_backward(int64_t N, int32_t degree, int32_t K_head, int32_t K_tail, const float *means, const float *head,
                          const float *tail, const float *campos_host, const float *v_colors, float *v_head, float *v_tail,
                          float *v_means, void *stream)
{
    if (int rc = check_sh_tables("sh_eval_backward", N, degree, K_head, K_tail, means, head, tail, campos_host))
        return rc;
    if (!v_head && !v_tail && !v_means)
        return set_error(GWBP_EINVAL, "sh_eval_backward: every output (v_head, v_tail, v_means) is null");
    if (v_tail && K_tail == 0)
        return set_error(GWBP_EINVAL, "sh_eval_backward: v_tail with K_tail = 0");
    if (N > 0 && !v_colors)
        return set_error(GWBP_EINVAL, "sh_eval_backward: null v_colors");
    if (misaligned(v_colors, 3) || misaligned(v_head, 3) || misaligned(v_tail, 3) || misaligned(v_means, 3))
        return set_error(GWBP_EINVAL, "sh_eval_backward: v_colors, v_head, v_tail and v_means must be 4-B aligned");
    const void *written[3];
    int n_written = 0;
    for (const void *p : {(const void *)v_head, (const void *)v_tail, (const void *)v_means})
        if (p)
            written[n_written++] = p;
    const void *const read[] = {means, head, tail, v_colors};
    if (N > 0)
        if (int rc = check_regions_distinct("sh_eval_backward", written, n_written, read, 4))
            return rc;
    return launch_sh_eval_bwd(N, degree, K_head, K_tail, means, head, tail, campos_host, v_colors, v_head, v_tail, v_means,
                              as_stream(stream));
}

// the same pair with the centre on the device (never dereferenced here), and the centre's gradient
int gwbp_sh_eval_dev(int64_t N, int32_t degree, int32_t K_head, int32_t K_tail, const float *means, const float *head,
                     const float *tail, const float *campos, float *out, void *stream)
{
    if (int rc = check_sh_tables("sh_eval_dev", N, degree, K_head, K_tail, means, head, tail, campos))
        return rc;
    if (N > 0 && !out)
        return set_error(GWBP_EINVAL, "sh_eval_dev: null out");
    if (misaligned(out, 3) || misaligned(campos, 3))
        return set_error(GWBP_EINVAL, "sh_eval_dev: campos and out must be 4-B aligned");
    const void *const written[] = {out}, *const read[] = {means, head, tail, campos};
    if (N > 0)
        if (int rc = check_regions_distinct("sh_eval_dev", written, 1, read, 4))
            return rc;
    return launch_sh_eval_dev(N, degree, K_head, K_tail, means, head, tail, campos, out, as_stream(stream));
}

int gwbp_sh_eval_backward_blocks(int64_t n_gaussians)
{
    if (n_gaussians < 0 || n_gaussians > 0x7FFFFFFF)
        return set_error(GWBP_EINVAL, "sh_eval_backward_blocks: %lld Gaussians out of range", (long long)n_gaussians);
    return sh_eval_backward_blocks(n_gaussians);
}

int gwbp_sh_eval_backward_dev(int64_t N, int32_t degree, int32_t K_head, int32_t K_tail, const float *means, const float *head,
                              const float *tail, const float *campos, const float *v_colors, float *v_head, float *v_tail,
                              float *v_means, double *v_campos, double *scratch, void *stream)
{
    if (int rc = check_sh_tables("sh_eval_backward_dev", N, degree, K_head, K_tail, means, head, tail, campos))
        return rc;
    if (!v_head && !v_tail && !v_means && !v_campos)
        return set_error(GWBP_EINVAL, "sh_eval_backward_dev: every output (v_head, v_tail, v_means, v_campos) is null");
    if (v_tail && K_tail == 0)
        return set_error(GWBP_EINVAL, "sh_eval_backward_dev: v_tail with K_tail = 0");
    if (N > 0 && !v_colors)
        return set_error(GWBP_EINVAL, "sh_eval_backward_dev: null v_colors");
    if (N > 0 && v_campos && !scratch)
        return set_error(GWBP_EINVAL, "sh_eval_backward_dev: v_campos needs the scratch (gwbp_sh_eval_backward_blocks(N) x 3 doubles)");
    if (misaligned(campos, 3) || misaligned(v_colors, 3) || misaligned(v_head, 3) || misaligned(v_tail, 3) || misaligned(v_means, 3))
        return set_error(GWBP_EINVAL, "sh_eval_backward_dev: campos, v_colors, v_head, v_tail and v_means must be 4-B aligned");
    if (misaligned(v_campos, 7) || misaligned(scratch, 7))
        return set_error(GWBP_EINVAL, "sh_eval_backward_dev: v_campos and scratch must be 8-B aligned");
    const void *written[5];
    int n_written = 0;
    for (const void *p : {(const void *)v_head, (const void *)v_tail, (const void *)v_means, (const void *)v_campos,
                          (const void *)(v_campos ? scratch : nullptr)})
        if (p)
            written[n_written++] = p;
    const void *const read[] = {means, head, tail, campos, v_colors};
    if (N > 0)
        if (int rc = check_regions_distinct("sh_eval_backward_dev", written, n_written, read, 5))
            return rc;
    return launch_sh_eval_bwd_dev(N, degree, K_head, K_tail, means, head, tail, campos, v_colors, v_head, v_tail, v_means, v_campos,
                                  scratch, as_stream(stream));
}

// ---- the optimiser step (adam.hip) ------------------------------------------------------------------------------------------------
int gwbp_adam_step(int64_t n, int32_t w, float *p, const float *g, float *m, float *v, const uint8_t *visible, float lr_over_bc1,
                   float sqrt_bc2, double b1, double b2, float eps, void *stream)
{
    if (int rc = check_densify_count("adam_step", n))
        return rc;
    if (w < 1)
        return set_error(GWBP_EINVAL, "adam_step: w must be at least 1 (got %d)", (int)w);
    if (!(lr_over_bc1 == lr_over_bc1) || !(sqrt_bc2 > 0.0f) || !(b1 >= 0.0 && b1 < 1.0) || !(b2 >= 0.0 && b2 < 1.0) || !(eps >= 0.0f))
        return set_error(GWBP_EINVAL, "adam_step: bad scalars (lr_over_bc1 %g, sqrt_bc2 %g > 0, b1 %g and b2 %g in [0, 1), eps %g >= 0)",
                         (double)lr_over_bc1, (double)sqrt_bc2, b1, b2, (double)eps);
    if (n > 0 && (!p || !g || !m || !v))
        return set_error(GWBP_EINVAL, "adam_step: null p, g, m or v");
    if (misaligned(p, 15) || misaligned(g, 15) || misaligned(m, 15) || misaligned(v, 15))
        return set_error(GWBP_EINVAL, "adam_step: p, g, m and v must be 16-B aligned");
    const void *const written[] = {p, m, v}, *const read[] = {g, visible};
    if (n > 0)
        if (int rc = check_regions_distinct("adam_step", written, 3, read, 2))
            return rc;
    return launch_adam_step(n, w, p, g, m, v, visible, lr_over_bc1, sqrt_bc2, b1, b2, eps, as_stream(stream));
}

// ---- the depth losses (depth_loss.hip) --------------------------------------------------------------------------------------------
// the render, its alpha map and the channel of all four entry points; `what` names the entry point
static int check_depth_image(const char *what, int32_t height, int32_t width, int32_t Dp, int32_t ch, const float *render,
                             const float *alpha)
{
    if (height < 1 || width < 1 || height > (1 << 24) || width > (1 << 24))
        return set_error(GWBP_EINVAL, "%s: an image of %d x %d pixels (width x height; each in [1, 2^24])", what, (int)width, (int)height);
    if ((int64_t)height * width > 0x7FFFFFFF)
        return set_error(GWBP_EINVAL, "%s: an image of %lld pixels (at most 2^31 - 1)", what, (long long)((int64_t)height * width));
    if (Dp < 1 || ch < 0 || ch >= Dp)
        return set_error(GWBP_EINVAL, "%s: channel %d of a render with %d channels", what, (int)ch, (int)Dp);
    if (!render || !alpha)
        return set_error(GWBP_EINVAL, "%s: null render or alpha", what);
    if (misaligned(render, 3) || misaligned(alpha, 3))
        return set_error(GWBP_EINVAL, "%s: render and alpha must be 4-B aligned", what);
    return GWBP_OK;
}

static int check_depth_points(const char *what, int64_t M, const float *points, const float *depths)
{
    if (M < 0 || M > 0x7FFFFFFF)
        return set_error(GWBP_EINVAL, "%s: bad number of points (%lld): 0 .. 2^31 - 1", what, (long long)M);
    if (M > 0 && (!points || !depths))
        return set_error(GWBP_EINVAL, "%s: null points or depths", what);
    if (misaligned(points, 3) || misaligned(depths, 3))
        return set_error(GWBP_EINVAL, "%s: points and depths must be 4-B aligned", what);
    return GWBP_OK;
}

static int check_depth_map(const char *what, const float *depth, const float *weights, int32_t kind)
{
    if (kind != GWBP_DEPTH_KIND_DISPARITY && kind != GWBP_DEPTH_KIND_DEPTH)
        return set_error(GWBP_EINVAL, "%s: unknown kind %d", what, (int)kind);
    if (!depth)
        return set_error(GWBP_EINVAL, "%s: null depth map", what);
    if (misaligned(depth, 3) || misaligned(weights, 3))
        return set_error(GWBP_EINVAL, "%s: the depth map and the weights must be 4-B aligned", what);
    return GWBP_OK;
}

// the outputs of a backward and the device scalar it reads
static int check_depth_grads(const char *what, const float *upstream, const float *v_render, const float *v_alpha)
{
    if (!upstream || !v_render || !v_alpha)
        return set_error(GWBP_EINVAL, "%s: null upstream, v_render or v_alpha", what);
    if (misaligned(upstream, 3) || misaligned(v_render, 3) || misaligned(v_alpha, 3))
        return set_error(GWBP_EINVAL, "%s: upstream, v_render and v_alpha must be 4-B aligned", what);
    return GWBP_OK;
}

static int check_depth_workspace(const char *what, const void *workspace, size_t workspace_bytes, size_t need)
{
    if (need == 0)
        return GWBP_OK;
    if (!workspace || misaligned(workspace, 7))
        return set_error(GWBP_EINVAL, "%s: null workspace, or one that is not 8-B aligned", what);
    if (workspace_bytes < need)
        return set_error(GWBP_EWORKSPACE, "%s: workspace has %zu bytes, needs %zu", what, workspace_bytes, need);
    return GWBP_OK;
}

int gwbp_depth_points_loss(int32_t height, int32_t width, int32_t Dp, int32_t ch, const float *render, const float *alpha, int64_t M,
                           const float *points, const float *depths, float scale, float *loss, float *per_point, void *workspace,
                           size_t workspace_bytes, void *stream)
{
    const char *what = "depth_points_loss";
    int rc = check_depth_image(what, height, width, Dp, ch, render, alpha);
    if (rc || (rc = check_depth_points(what, M, points, depths)))
        return rc;
    if (!loss || misaligned(loss, 3) || misaligned(per_point, 3))
        return set_error(GWBP_EINVAL, "%s: null loss, or a loss or per_point that is not 4-B aligned", what);
    if ((rc = check_depth_workspace(what, workspace, workspace_bytes, depth_points_workspace_bytes(M))))
        return rc;
    return launch_depth_points_loss(height, width, Dp, ch, render, alpha, M, points, depths, scale, loss, per_point,
                                    static_cast<double *>(workspace), as_stream(stream));
}

int gwbp_depth_points_backward(int32_t height, int32_t width, int32_t Dp, int32_t ch, const float *render, const float *alpha,
                               int64_t M, const float *points, const float *depths, float scale, const float *upstream,
                               float *v_render, float *v_alpha, void *stream)
{
    const char *what = "depth_points_backward";
    int rc = check_depth_image(what, height, width, Dp, ch, render, alpha);
    if (rc || (rc = check_depth_points(what, M, points, depths)) || (rc = check_depth_grads(what, upstream, v_render, v_alpha)))
        return rc;
    const void *const written[] = {v_render, v_alpha}, *const read[] = {render, alpha, points, depths, upstream};
    if ((rc = check_regions_distinct(what, written, 2, read, 5)))
        return rc;
    return launch_depth_points_backward(height, width, Dp, ch, render, alpha, M, points, depths, scale, upstream, v_render, v_alpha,
                                        as_stream(stream));
}

int gwbp_depth_map_loss(int32_t height, int32_t width, int32_t Dp, int32_t ch, const float *render, const float *alpha,
                        const float *depth, const float *weights, int32_t kind, float scale, float *loss, double *sums,
                        void *workspace, size_t workspace_bytes, void *stream)
{
    const char *what = "depth_map_loss";
    int rc = check_depth_image(what, height, width, Dp, ch, render, alpha);
    if (rc || (rc = check_depth_map(what, depth, weights, kind)))
        return rc;
    if (!loss || !sums || misaligned(loss, 3) || misaligned(sums, 7))
        return set_error(GWBP_EINVAL, "%s: null loss or sums, or a loss that is not 4-B or sums that are not 8-B aligned", what);
    if ((rc = check_depth_workspace(what, workspace, workspace_bytes, depth_map_workspace_bytes(height, width))))
        return rc;
    return launch_depth_map_loss(height, width, Dp, ch, render, alpha, depth, weights, kind, scale, loss, sums,
                                 static_cast<double *>(workspace), as_stream(stream));
}

int gwbp_depth_map_backward(int32_t height, int32_t width, int32_t Dp, int32_t ch, const float *render, const float *alpha,
                            const float *depth, const float *weights, int32_t kind, float scale, const double *sums,
                            const float *upstream, float *v_render, float *v_alpha, void *stream)
{
    const char *what = "depth_map_backward";
    int rc = check_depth_image(what, height, width, Dp, ch, render, alpha);
    if (rc || (rc = check_depth_map(what, depth, weights, kind)) || (rc = check_depth_grads(what, upstream, v_render, v_alpha)))
        return rc;
    if (!sums || misaligned(sums, 7))
        return set_error(GWBP_EINVAL, "%s: null sums, or sums that are not 8-B aligned", what);
    const void *const written[] = {v_render, v_alpha}, *const read[] = {render, alpha, depth, weights, upstream, sums};
    if ((rc = check_regions_distinct(what, written, 2, read, 6)))
        return rc;
    return launch_depth_map_backward(height, width, Dp, ch, render, alpha, depth, weights, kind, scale, sums, upstream, v_render,
                                     v_alpha, as_stream(stream));
}

int gwbp_accumulate_stats(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, gwbp_stats *accum,
                          void *stream)
{
    Layout L;
    Ws W;
    int rc = bind_workspace(caps, workspace, workspace_bytes, &L, &W);
    if (rc)
        return rc;
    if (!accum)
        return set_error(GWBP_EINVAL, "null accum");
    return launch_accum_stats(W, accum, as_stream(stream));
}

int gwbp_read_stats(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, gwbp_stats *stats_host,
                    void *stream)
{
    Layout L;
    Ws W;
    int rc = bind_workspace(caps, workspace, workspace_bytes, &L, &W);
    if (rc)
        return rc;
    if (!stats_host)
        return set_error(GWBP_EINVAL, "null stats_host");
    hipStream_t s = as_stream(stream);
    if ((rc = check_hip(hipMemcpyAsync(stats_host, W.counters, sizeof(gwbp_stats), hipMemcpyDeviceToHost, s),
                        "stats copy")))
        return rc;
    return check_hip(hipStreamSynchronize(s), "stats sync");
}

int gwbp_dump_pairs(const gwbp_caps *caps, void *workspace, size_t workspace_bytes, const gwbp_view *view_host,
                    int64_t cap, int32_t *gid, int32_t *pix, float *w, int64_t *n_host, void *stream)
{
    Bound B;
    int rc = bind(caps, workspace, workspace_bytes, view_host, stream, &B);
    if (rc)
        return rc;
    if (!n_host || cap < 0 || (cap > 0 && (!gid || !pix || !w)))
        return set_error(GWBP_EINVAL, "bad dump arguments");
    // scratch counter: reuse digit_total[0..1] (free once the sort has finished)
    u64 *n_dev = reinterpret_cast<u64 *>(B.W.digit_total);
    if ((rc = check_hip(hipMemsetAsync(n_dev, 0, sizeof(u64), B.s), "dump memset")))
        return rc;
    if ((rc = launch_dump_pairs(B.L, B.W, B.V, cap, gid, pix, w, n_dev, B.s)))
        return rc;
    u64 n = 0;
    if ((rc = check_hip(hipMemcpyAsync(&n, n_dev, sizeof(u64), hipMemcpyDeviceToHost, B.s), "dump copy")))
        return rc;
    if ((rc = check_hip(hipStreamSynchronize(B.s), "dump sync")))
        return rc;
    *n_host = (int64_t)n;
    return GWBP_OK;
}

} // extern "C"
