// mask_features.h -- the slot store and kernel arguments of gwbp_scatter_mask_features (mask_features.hip).
//
// A mask-pooled feature map is a label map L [H, W] plus one row per label of a table E [M, D]; the per-pixel map E[L] is
// piecewise constant, so
//     F[g, :] += scale_f * sum_k s_{g,k} E[k, :],     s_{g,k} = sum_{p : L(p) = k} w_g(p),     d[g] += scale_d * sum_p w_g(p)
// -- token space (token.hip) with data-dependent token ids.  The per-(Gaussian, tile) label sums are filed at the record's EMIT
// position (k_emit: a Gaussian's intersections lie back to back, row-major over its tile rectangle, from estart[gid]), where one
// wave per Gaussian reads them back to back.
#pragma once

#include "gwbp_dev.h"

namespace gwbp {

constexpr int kMaskSlots = 4; // (label, sum) slots per emit position; a record with more distinct labels spills the rest
static_assert(kMaskSlots * 8 == GWBP_MASK_SLOT_BYTES, "gwbp.h's slot size");

// The caller's slot store, isect_cap emit positions: labels [isect_cap][kMaskSlots] int32 (-1 = weight outside [0, M): counts
// in d only), then sums [isect_cap][kMaskSlots] fp32.  Only the sums are cleared per view (an emit position without a record
// reads as four zero sums); a label is read only where its sum is non-zero.
struct MaskSlots {
    int4 *labels;
    float4 *sums;
};

struct MaskApplyArgs {
    int64_t N;
    const u32 *order;   // Gaussians in depth order (the emit order)
    const u32 *touched; // emit positions per Gaussian (0 = culled)
    const u32 *estart;  // first emit position
    const int *labels;  // MaskSlots, as flat arrays
    const float *sums;
    const void *table; // table[k * ts_row + c] (elements of the kernel's table type)
    int64_t ts_row;
    int D;
    int n_pass; // passes over the channels, 256 NC each
    float scale_f, scale_d;
    float *F, *d;
    Counters *ctr;
};

int launch_mask_features(const Layout &L, const Ws &W, const ViewDev &V, const void *labels, int label_type, int64_t ls_y,
                         int64_t ls_x, const int32_t *ymap, const int32_t *xmap, const void *table, int table_type,
                         int64_t ts_row, int M, int D, float scale_f, float scale_d, float *F, float *d, const MaskSlots &S,
                         u32 *n_spilled, hipStream_t s);

} // namespace gwbp
