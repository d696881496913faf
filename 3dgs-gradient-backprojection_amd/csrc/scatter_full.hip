// scatter_full.hip -- k_scatter_full: the D % 128 == 0 (and D <= 64) fast path of the weighted scatter-accumulate
// (C2/C4/C5-input: D = 512 / 768 / 1024; dino 384); semantics identical to k_scatter (scatter.hip).  Channel-contiguous
// maps are staged with 16-B loads, any other strides element-wise; optional row/column maps address a low-resolution
// feature map (nearest upsampling, backproject.py:244-248).
//
//   F[g, c0:c0+128] += sum_p w_g(p) * feats[p, c0:c0+128]        (backproject.py:127-131 via colors.grad)
//
// work item = (16x16 tile, 128-channel chunk); 1024 threads = 16 waves, ONE PERSISTENT workgroup per CU (128 KB LDS)
// pulling items from a per-XCD-class queue:
//   * the tile's 256 px x 128 ch slab is staged once (eight 16-B loads per thread in flight, then eight LDS writes):
//     every feature byte is read from HBM exactly once per view
//   * a wave owns one (Gaussian, tile) record at a time (LDS work counter); the Gaussian is wave-uniform and
//     lanes = channel pairs (ds_read_b64: conflict-free 512-B rows)
//   * the record's {w, pixel} entries are contiguous in the weight store (k_blend writes a record's four quarter
//     lists back to back): lane s of load j fetches entry 64j + s with one 8-B load, so a typical record
//     (45 entries) costs ONE coalesced 512-B load.  The accumulate loop walks the entries in batches of 8 with
//     compile-time lane selects: per pair 2 v_readlane (w, pixel) + 1 v_lshl_add (LDS address) + 1 ds_read_b64 +
//     1 v_pk_fma_f32; the next batch's eight LDS reads are issued before the current batch's FMAs.
//     Measured ceiling of exactly this instruction mix (tools/ubench_scatter.hip, 16 waves/CU): 453 pairs/us/CU
//     = 2.98 ms per C2 view; ds_read_b64 + v_pk_fma alone: 1.86 ms.
//   * records are software-pipelined: claim + header scalar loads two records ahead, entry loads one record ahead.
//     The entry loads are inline asm and awaited with a COUNTED s_waitcnt: vmcnt retires in order and a float atomic
//     stays counted for ~3000 cycles under load, so the vmcnt(0) hipcc would insert in front of every record's
//     entries serialised each record behind its predecessor's atomics (first profile: 7.2 ms/view).
//         [loads(i): 2] [atomics(i-1): 2 F (+1 d)] [loads(i+1): 2]   ->   s_waitcnt vmcnt(4)
//     Every VMEM instruction in the steady-state loop is unconditional, so 4 is a guaranteed lower bound of the
//     younger operations (an over-wait is always safe).
//   * flush: channel pairs are transposed across lanes (ds_bpermute) so each of the two atomic wave-instructions
//     covers 64 consecutive dwords (256 contiguous bytes: the shape that runs at the full fp32 atomic rate)
#include "scatter_full_kernel.h"

namespace gwbp {

int launch_scatter_full(const Layout &L, const Ws &W, const ViewDev &V, const FeatMap &M, int D, float scale_f,
                        float scale_d, float *F, float *d, hipStream_t s)
{
    const bool small = D <= 64;
    // 16-B vector staging needs channel-contiguous, 16-B aligned pixel rows
    const bool aligned = M.fs_c == 1 && (M.fs_x % 4 == 0) && (M.fs_y % 4 == 0) &&
                         ((reinterpret_cast<uintptr_t>(M.p) & 15) == 0);
    const int vec_ok = aligned ? (M.bilinear() ? 2 : 1) : 0; // 1: 16-B staging, 2: 16-B bilinear staging, 0: element-wise
    const int n_chunks = small ? 1 : D / kChunk;
    const int pitch = small ? ((D + 3) & ~3) : kChunk;
    const bool enc = M.enc != nullptr;
    if (enc && (!small || D > kEncN || M.enc_k < 16 || (M.enc_k & 15) || M.enc_k > 1024 || !aligned || M.bilinear() || M.ymap))
        return set_error(GWBP_EINVAL, "fused encoder needs D <= 16, K %% 16 == 0, K <= 1024 and a plain channel-contiguous map");
    // slab + work counter + two item slots (+ the encoder table for the fused-encoder staging)
    const size_t lds_bytes = (size_t)kTilePix * pitch * sizeof(float) + 16 + (enc ? (size_t)M.enc_k * kEncN * sizeof(float) : 0);
    const void *fns[4] = {reinterpret_cast<const void *>(k_scatter_full<false, 0, GWBP_MAP_F32>),
                          reinterpret_cast<const void *>(k_scatter_full<false, 1, GWBP_MAP_F32>),
                          reinterpret_cast<const void *>(k_scatter_full<false, 2, GWBP_MAP_F32>),
                          reinterpret_cast<const void *>(k_scatter_full<true, 0, GWBP_MAP_F32>)};
    for (int i = 0; i < 4; ++i) {
        const int rc = ensure_dynamic_lds(fns[i], i < 3 ? (int)kLdsBytes : 65536 + 16);
        if (rc)
            return rc;
    }
    if (enc) {
        const int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(k_scatter_full<true, 3, GWBP_MAP_F32>), 16384 + 16 + 1024 * kEncN * 4);
        if (rc)
            return rc;
    }
    int n_cu = 0;
    {
        const int rc = device_cus(&n_cu);
        if (rc)
            return rc;
    }
    // persistent workgroups: one per CU (two for the small-D path whose slab is <= 64 KB); caps.scatter_workgroups
    // overrides; always a multiple of the 8 XCD classes
    int grid = L.scatter_wgs > 0 ? L.scatter_wgs : (small ? 2 * n_cu : n_cu);
    grid = (grid + 7) & ~7;
    u32 *queues = W.shards + kShards * 16;
    const int dbg = profile_knob("GWBP_ABLATE");
#define GWBP_LAUNCH(S, Vc)                                                                                            \
    hipLaunchKernelGGL((k_scatter_full<S, Vc, GWBP_MAP_F32>), dim3(grid), dim3(kThreads), lds_bytes, s, V, n_chunks, W.tile_offsets,  \
                       W.hdr_count, W.headers, W.wpool, M, pitch, D, scale_f, scale_d, F, d, queues, dbg)
    if (enc)
        GWBP_LAUNCH(true, 3);
    else if (small)
        GWBP_LAUNCH(true, 0);
    else if (vec_ok == 1)
        GWBP_LAUNCH(false, 1);
    else if (vec_ok == 2)
        GWBP_LAUNCH(false, 2);
    else
        GWBP_LAUNCH(false, 0);
#undef GWBP_LAUNCH
    return check_hip(hipGetLastError(), "scatter_full launch");
}

} // namespace gwbp
