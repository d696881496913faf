// token.hip -- the scatter of a NEAREST-UPSAMPLED low-resolution map in TOKEN space (dino variant, backproject.py:242-289).
//
// The reference upsamples the network's 64 x 64 x 1024 patch-token map to the view's 1600 x 1060 pixels with
// F.interpolate(mode="nearest") (backproject.py:244-248) and back-projects the 6.9 GB result.  Every pixel of a token carries the
// same vector, so
//     F_v[g, :] = sum_p w_g(p) feats[p, :] = sum_t omega_{g,t} tok[t, :],     omega_{g,t} = sum_{p in t} w_g(p),
// and when a token is at least a tile wide and high a 16 x 16 tile sees at most 2 x 2 of them: k_blend<kToken> (blend.hip) reduces
// every contributing (Gaussian, tile) record to FOUR weight sums and files them at the record's EMIT position.  k_emit wrote the
// intersections of one Gaussian contiguously (row-major over its tile rectangle, Gaussians in depth order), so here one wave
// walks a Gaussian's sums back to back, multiplies them with token rows and adds the result to F[g, :] with ONE plain
// read-modify-write per view -- the formulation "whose partial sums are combined on chip across tiles" that the full-resolution
// path cannot have, available because the D-wide operand is a 16 MB table instead of a 6.9 GB map:
// no atomics, no weight store, no slabs, no carry rows, no sort by Gaussian.
//
// HBM traffic per view: 8 B x D per Gaussian that receives weight (C2 geometry, D = 1024: 0.53 M rows -> 4.4 GB) + the 16-B sums
// (0.06 GB); the token rows (about five 4-KB rows per touched Gaussian) come from LDS, the few outside the window from L2.
//
// Work map (k_token_apply<NC, true, FULL>, the product): a workgroup of four waves takes 256 consecutive entries of the
// (tile, depth)-sorted intersection list and works on the Gaussians whose HOME tile -- first tile of their rectangle, emit slot 0 --
// is the entry's tile: every Gaussian exactly once, neighbours on the screen back to back.  The 3 x 3 token rows under the first
// entry's tile are staged in LDS (per pass over the channels: 9 x 256 NC floats); a Gaussian's rectangle of up to 2 x 2 tiles reaches at most three token columns
// and rows, so almost every token read is an LDS read.  A wave first finds, lane-parallel, which of its Gaussians carry weight at
// all, then walks those with two register sets: the NEXT Gaussian's F row, first 16 sums and d are requested (unconditionally, so
// that the waits are counted ones) before the current one is multiplied out and stored -- a row's read, its write and the next
// row's read are all in flight together.
//
// Measured per C2-geometry view at D = 1024, alone / in the pipeline, same box each step (profiles/r6_token_*.txt, DESIGN.md
// section 9): first version -- one (Gaussian, 256-channel chunk) per wave iteration, chunk tied to the XCD -- 2.17 ms; one wave
// per Gaussian over all channels in depth order 1.27 / 1.85; tile order + LDS window 1.07 / 1.73; + the request one Gaussian
// ahead 0.87 / 1.42 (4.45 GB of 4-KB rows read and written at 5.1 TB/s).  Depth order (k_token_apply<NC, false, FULL>) stays as
// the -DGWBP_TOKEN_DEPTH_ORDER A/B build.  Channels: 256-channel chunks, up to four side by side per pass, as few passes as that
// allows (D = 1024: 1 x 4; 1536: 2 x 3; 384: 1 x 2 with half a chunk masked off) -- any D % 4 == 0.  Tried and dropped: XCD-local channel groups (1.32-1.66 alone), tile order without the window (no gain:
// the L2 gathers did not bind, the per-Gaussian latency chain did), a 2 x 2 register window, channel-group waves.
#include "token_kernel.h"

namespace gwbp {

__global__ __launch_bounds__(256) void k_zero_omega(float4 *__restrict__ omega, const Counters *__restrict__ ctr, int prio)
{
    front_priority(prio);
    const u32 n = ctr->n_isect;
    for (u32 i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u)
        omega[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}

int launch_zero_omega(const Layout &L, const Ws &W, hipStream_t s)
{
    const int prio = (L.flags & GWBP_FLAG_FRONT_PRIORITY) ? 1 : 0;
    hipLaunchKernelGGL(k_zero_omega, dim3(1024), dim3(256), 0, s, reinterpret_cast<float4 *>(W.headers), W.counters, prio);
    return check_hip(hipGetLastError(), "zero_omega launch");
}

int launch_token_apply(const Layout &L, const Ws &W, const ViewDev &V, const float *tokens, int64_t ts_y, int64_t ts_x, int D,
                       const int32_t *ymap, const int32_t *xmap, float scale_f, float scale_d, float *F, float *d, hipStream_t s)
{
    return launch_token_apply_t<GWBP_MAP_F32>(L, W, V, tokens, ts_y, ts_x, D, ymap, xmap, scale_f, scale_d, F, d, s);
}

} // namespace gwbp
