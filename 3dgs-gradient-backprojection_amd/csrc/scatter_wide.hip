// scatter_wide.hip -- k_scatter_wide: the D % 256 == 0, channel-contiguous path of the weighted scatter-accumulate
// (C2 D = 512, C4 D = 768, dino-sized 1024); semantics identical to k_scatter / k_scatter_full.
//
//   F[g, c0:c0+256] += sum_p w_g(p) * feats[p, c0:c0+256]        (backproject.py:127-131 via colors.grad)
//
// Why a second fast path: k_scatter_full spends 4 vector instructions per (pair, 128 channels) -- 2 v_readlane,
// 1 address add, 1 v_pk_fma_f32.  With 4 channels per lane (ds_read_b128 + 2 v_pk_fma_f32) the two v_readlane and the
// address add are shared by 256 channels: 2.5 instructions per (pair, 128 channels).  The price is LDS capacity:
// 256 px x 256 ch x 4 B does not fit, so a work item = (tile, 256-channel chunk) runs in TWO passes over half-tile slabs
// (tile rows 0..7, then 8..15; 128 px x 256 ch = 128 KB each).  The flush traffic must not grow with it -- fp32 atomics
// run memory-side at ~1.3 TB/s chip-wide and the per-(Gaussian, tile) flush sits right at that rate (profiles/
// r4_wide_ablation.txt) -- so a record with entries in both halves is NOT flushed twice: the top pass parks its partial
// sums in a carry row (plain stores into a per-workgroup slice), the bottom pass starts from them and issues the one
// atomic flush.
//
// Slab layout: row = pixel (1 KB), position 4*l + k of a row holds channel c0 + 64*k + l.  Lane l reads its 16 B with
// one conflict-free ds_read_b128 and owns channels {l, l+64, l+128, l+192}: the flush is four 256-B contiguous
// atomic wave-instructions with no cross-lane transpose.
//
// Round 4 rewrite of the visit machinery (the arithmetic and the order of every record's sum are unchanged):
//   * The pass's visit list is built BY THIS KERNEL, in LDS, from the blend's 64-B record headers while the slab loads are
//     in flight (thread i takes record i, a ballot compacts the records that have entries in this half): the blend no
//     longer writes half-tile lists, and a visit's descriptor is one broadcast ds_read_b96 (a scalar load of it would have forced
//     every lgkmcnt wait of the loop to zero; the ONE scalar load per batch that round 5 put into the loop is accounted for
//     in the batch's counted waits, see GWBP_BATCH_ASM).
//   * Claims are asynchronous: the ds_add_rtn for the visit after next is issued at the top of a visit and read after its
//     first batch; the descriptor read it enables completes under the rest of the visit.
//   * Every VMEM operation of a visit addresses SGPR base + one of two per-lane constants (lane * 4 / 8): no vector
//     address arithmetic, no 64-bit VGPR pairs.
//   * One landing buffer: the carry dwords of the next visit (and the L2 warm-up of its entries) are loaded a whole visit
//     ahead, consumed by the selects that start a visit, and only then re-targeted.  One copy of the visit code per pass.
// Round 5: the entries reach the arithmetic through the SCALAR unit.  A batch of eight pairs is ONE s_load_dwordx16 into an
// aligned SGPR tuple -- entry j = the SGPR pair {w, pix}: v_pk_fma_f32 reads the weight and v_lshl_add_u32 the pixel straight from
// it -- so a pair costs 3 vector instructions (address, two packed FMAs) where rounds 1-4 spent 5 (two v_readlane in front).  The
// structure-preserving ablation had priced the two v_readlane at 5 % of the C2 step, 10 % together with fewer flushes
// (profiles/r5_combined_ablation.txt); round 1 had found scalar-fed entries latency-bound (8.9 ms).  What makes them stream
// (tools/ubench_sload.hip): (i) the visit's lines are pulled into L2 a whole visit ahead by a one-dword-per-line vector load, so
// the scalar load is an L2 hit; (ii) a rolling double buffer of two fixed SGPR tuples, s[68:83] and s[84:99], which the
// compiler never allocates (amdgpu_num_sgpr(76) keeps it inside s0..s67; a CPU test scans the assembly): the load of batch
// b + 1 -- at the end of a visit: the NEXT visit's first batch -- goes out at the top of batch b and has landed when batch b's last
// FMA has waited for lgkmcnt(0); nothing of the stream is ever in flight outside a batch's asm block.  The blend pads both
// half-tile lists of a record to eight entries with {0, kPadPix} (gwbp_dev.h: Header), so a batch needs no remainder handling.
// The batch loop is a run-time loop over two copies of the block (tuple A -> B, B -> A): 6 KB of code where the unrolled
// v_readlane form had 20.
// Every VMEM instruction of a visit is unconditional WITHIN a pass, so the counted s_waitcnt in front of a visit's carry dwords
// is exact: a visit issues its loads (1 warm-up in the top pass, 1 + 4 carry dwords in the bottom pass) and 4 flush operations
// (atomics, or the 4 stores that park a spanning record).  The denominator d is not accumulated here: the blend adds
// every record's weight sum to d itself (gwbp_blend_weights_d), or k_accum_d (scatter.hip) does from the headers.


#include "gwbp_dev.h"

#ifdef GWBP_STAMPS
namespace gwbp {
__device__ unsigned long long g_wide_prof[8];
}
#endif

#include "scatter_wide_kernel.h"

namespace gwbp {

#ifdef GWBP_STAMPS
extern "C" int gwbp_profile_read_wide(unsigned long long *out8_host)
{
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyFromSymbol(out8_host, HIP_SYMBOL(g_wide_prof), sizeof(z)) != hipSuccess)
        return -1;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_wide_prof), z, sizeof(z)) == hipSuccess ? 0 : -1;
}
#endif

int launch_scatter_wide(const Layout &L, const Ws &W, const ViewDev &V, const FeatMap &M, int D, float scale_f,
                        float *F, hipStream_t s)
{
    return launch_scatter_wide_t<GWBP_MAP_F32>(L, W, V, M, D, scale_f, F, s);
}

} // namespace gwbp
