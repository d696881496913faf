"""The yardstick of the blend backward ALONE (k_render_px_bwd, gwbp_render_pixels_backward): one view's blend restated in torch on
the tile lists, in any dtype, from the projected records as they were filed.

tests/raster_grad_ref.py restates the whole of rasterization() in one dense [H*W, N] table and starts from means, quats and scales:
its float32 floor is the rounding of the projected records, and an image of a few hundred tiles does not fit it.  This one starts
BEHIND the projection: the float32 records (means2d [N, 2], conics [N, 3], the filed opacity [N] -- already times the antialiasing
compensation), the sorted tile lists (flatten_ids, tile_offsets) and the set of valid (pixel, Gaussian) pairs are inputs, so the
kernel and the float64 run read the same numbers and record rounding drops out of both sides.  WHICH pairs count is never decided
here (alpha >= 1/255, sigma >= 0, the T <= 1e-4 termination): the pairs come from the blend that was run (blend_weights +
dump_pairs on the device, the CPU oracle's blend_pairs without one).

Per non-empty tile, a dense [256, L] table over that tile's own list, in list order (tiles of similar length are padded to one
[B, 256, L] batch; a padded entry is outside the mask), on the mask

    sigma = 0.5 (ca dx^2 + cc dy^2) + cb dx dy,  dx = mx - (x + 0.5),  dy = my - (y + 0.5)
    alpha = min(0.999, o exp(-sigma)),  T = exclusive cumulative product of (1 - alpha) along the list
    out = sum alpha T c,  alpha_img = 1 - T_end

and torch.autograd.grad of sum(out v_out) + sum(alpha_img v_alpha) with the batch's records and colours as leaves, added over the
tiles into v_g2d [N, 6] = d / d(mx, my, ca, cb, cc, o) and v_colors [N, D].  Empty tiles are skipped: an image of 80 000 tiles with
a few thousand filled ones costs what those cost.  The float64 run is the truth; the float32 run of the same code from the same
records is the floor the kernel is measured in.
"""
import numpy as np
import torch

import raster_grad_ref as rg

TILE = 16
ALPHA_MAX = rg.ALPHA_MAX
COLUMNS = ("mx", "my", "ca", "cb", "cc", "o")
QUANTITIES = COLUMNS + ("colors",)
ROW_GROUPS = (("mean", slice(0, 2)), ("conic", slice(2, 5)), ("opacity", slice(5, 6)))  # the v_g2d columns of each row figure
BATCH_ENTRIES = 1 << 21  # [B, 256, L] entries per batch
STACK_TILE = 1           # tile (1, 0) of the 3 x 2 tiles of test_gpu_raster_grad._stack's 37 x 21 image
# The stack of 600 at these opacities, chosen with the CPU oracle's cut: T falls to 1e-4 at a different list position for more than
# a hundred of the tile's pixels, on both sides of the first staging batch of 256.  At 0.15 the last records lie at positions
# 164 .. 537 (counted from 1, as the kernel's `last`): pixels end in all three batches and n_used is strictly inside the third; at
# 0.2 at 120 .. 386: n_used strictly inside the second.  (At 0.04 .. 0.08 nobody ends before position 319, and at 0.02 nobody
# terminates.)  tests/test_blend_grad_ref_cpu.py asserts this on the oracle's cut, tests/test_gpu_blend_grad.py on the kernel's.
TERMINATION_OPACITIES = (0.15, 0.2)


def nobody_terminates(ref, max_opacity):
    """From a float64 blend() of the cut: no pixel of the view has terminated.  A pixel terminates at the record that would take its
    T to 1e-4 or below and keeps the T in front of it, so a terminated pixel ends with T (1 - alpha) <= 1e-4, alpha <= max_opacity:
    every T_end above 1e-4 / (1 - max_opacity) belongs to a pixel that walked its whole list."""
    return float((1.0 - ref["alpha_img"]).min()) > 1.01e-4 / (1.0 - max_opacity)


def check_termination(pl, n=600):
    """The conditions of the termination scenes, from a cut: (smallest, largest last position counted from 1, distinct values)."""
    last = last_positions(pl, STACK_TILE) + 1
    assert list_length(pl, STACK_TILE) == n and int(last.min()) >= 1
    lo, hi, kinds = int(last.min()), int(last.max()), len(torch.unique(last))
    assert lo <= 256 < hi, (lo, hi)                      # pixels of one tile whose last record lies in different batches
    assert int((last <= 256).sum()) >= 10 and int((last > 256).sum()) >= 10
    assert kinds >= 10, kinds
    assert hi < n and hi % 256 not in (0, 1), hi         # n_used inside a batch: not at the list's end, not at a batch's
    return lo, hi, kinds


def _i64(a):
    return torch.as_tensor(np.asarray(a.detach().cpu() if torch.is_tensor(a) else a)).to(torch.int64).reshape(-1)


def plan(flatten_ids, tile_offsets, gid, pix, W, H, n_gaussians):
    """What both dtypes share: dict(W, H, n, batches, paired bool [N]); a batch = dict(tiles [B], ids [B, L] (0 where padded),
    lens [B], mask bool [B, 256, L], px / py int64 [B, 256], inside bool [B, 256], pixel int64 [B, 256] (0 outside the image)).
    flatten_ids: at least tile_offsets[-1] entries.  Every (gid, pix) pair must name a Gaussian of its pixel's tile list."""
    offs, flat = _i64(tile_offsets), _i64(flatten_ids)
    gid, pix = _i64(gid), _i64(pix)
    tw, th = -(-W // TILE), -(-H // TILE)
    assert offs.numel() == tw * th + 1 and int(offs[0]) == 0 and flat.numel() >= int(offs[-1])
    flat = flat[:int(offs[-1])]
    lens = offs[1:] - offs[:-1]
    # list position of each pair: (tile, Gaussian) is unique among the intersections
    tile_of = torch.repeat_interleave(torch.arange(tw * th), lens)
    key = tile_of * n_gaussians + flat
    key_sorted, where = torch.sort(key)
    assert key_sorted.numel() < 2 or bool((key_sorted[1:] > key_sorted[:-1]).all()), "a Gaussian twice in one tile list"
    x, y = pix % W, pix // W
    ptile = (y // TILE) * tw + x // TILE
    pkey = ptile * n_gaussians + gid
    at = torch.searchsorted(key_sorted, pkey).clamp_(max=max(key_sorted.numel() - 1, 0))
    assert pkey.numel() == 0 or bool((key_sorted[at] == pkey).all()), "a pair whose Gaussian is not in its pixel's tile list"
    pos = where[at] - offs[ptile]
    local = (y % TILE) * TILE + x % TILE
    filled = torch.nonzero(lens > 0).reshape(-1)
    filled = filled[torch.argsort(lens[filled], stable=True)]
    slot_of = torch.full((tw * th,), -1, dtype=torch.int64)  # (batch, row) of a filled tile, as batch * 2^32 + row
    batches, i = [], 0
    ar = torch.arange(TILE * TILE)
    while i < filled.numel():
        j = i + 1
        while j < filled.numel() and (j + 1 - i) * TILE * TILE * int(lens[filled[j]]) <= BATCH_ENTRIES:
            j += 1
        tiles = filled[i:j]
        L = int(lens[tiles].max())
        col = torch.arange(L)[None, :]
        real = col < lens[tiles][:, None]
        ids = torch.where(real, flat[(offs[tiles][:, None] + col).clamp_(max=flat.numel() - 1)], torch.zeros((), dtype=torch.int64))
        px = (tiles % tw)[:, None] * TILE + (ar % TILE)[None, :]
        py = (tiles // tw)[:, None] * TILE + (ar // TILE)[None, :]
        inside = (px < W) & (py < H)
        slot_of[tiles] = len(batches) * (1 << 32) + torch.arange(j - i)
        batches.append(dict(tiles=tiles, ids=ids, lens=lens[tiles], mask=torch.zeros(j - i, TILE * TILE, L, dtype=torch.bool),
                            px=px, py=py, inside=inside, pixel=torch.where(inside, py * W + px, torch.zeros_like(px))))
        i = j
    slot = slot_of[ptile]
    for b, bt in enumerate(batches):
        sel = (slot >> 32) == b
        bt["mask"][slot[sel] & 0xFFFFFFFF, local[sel], pos[sel]] = True
    paired = torch.zeros(n_gaussians, dtype=torch.bool)
    paired[gid] = True
    return dict(W=W, H=H, n=n_gaussians, batches=batches, paired=paired)


def last_positions(pl, tile):
    """int64 [256]: list position of the last valid record of each pixel of `tile`, -1 for a pixel that takes none."""
    for bt in pl["batches"]:
        hit = torch.nonzero(bt["tiles"] == tile).reshape(-1)
        if hit.numel():
            m = bt["mask"][int(hit[0])]
            L = m.shape[1]
            return torch.where(m.any(dim=1), L - 1 - m.flip(1).float().argmax(dim=1), torch.full((m.shape[0],), -1))
    return torch.full((TILE * TILE,), -1)


def list_length(pl, tile):
    for bt in pl["batches"]:
        hit = torch.nonzero(bt["tiles"] == tile).reshape(-1)
        if hit.numel():
            return int(bt["lens"][int(hit[0])])
    return 0


def _blend_batch(bt, m2d, con, opa, col, dt):
    """(out [B, 256, D], alpha_img [B, 256]) of one batch from its gathered records [B, L, .]."""
    mask = bt["mask"]
    dx = m2d[:, None, :, 0] - (bt["px"].to(dt) + 0.5)[:, :, None]
    dy = m2d[:, None, :, 1] - (bt["py"].to(dt) + 0.5)[:, :, None]
    sigma = 0.5 * (con[:, None, :, 0] * dx * dx + con[:, None, :, 2] * dy * dy) + con[:, None, :, 1] * dx * dy
    sigma = torch.where(mask, sigma, torch.zeros_like(sigma))  # (no exp of what the mask drops: inf * 0 in its gradient)
    raw = torch.where(mask, opa[:, None, :] * torch.exp(-sigma), torch.zeros_like(sigma))
    alpha = torch.clamp(raw, max=ALPHA_MAX)
    t_incl = torch.cumprod(1.0 - alpha, dim=2)
    t_excl = torch.cat([torch.ones_like(t_incl[:, :, :1]), t_incl[:, :, :-1]], dim=2)
    return torch.bmm(alpha * t_excl, col), 1.0 - t_incl[:, :, -1]


def blend(dtype, pl, means2d, conics, opacities, colors, v_out, v_alpha=None, skip=(), grads=True):
    """dict(out [H, W, D], alpha_img [H, W], loss, v_g2d [N, 6], v_colors [N, D]) in `dtype` (the gradients only with grads=True).
    The records and the colour table in any float dtype (float32 as filed: widening them is exact); v_alpha None = zeros.
    skip: (tile, list position) pairs whose gradient contribution is left out of the sums -- for a test that wants to know what
    a dropped record looks like."""
    W, H, n = pl["W"], pl["H"], pl["n"]
    rec = [torch.as_tensor(t).detach().cpu().to(dtype) for t in (means2d, conics, opacities, colors)]
    D = rec[3].shape[1]
    G = torch.as_tensor(v_out).detach().cpu().reshape(H * W, D)
    A = None if v_alpha is None else torch.as_tensor(v_alpha).detach().cpu().reshape(H * W)
    out, alpha_img = torch.zeros(H * W, D, dtype=dtype), torch.zeros(H * W, dtype=dtype)
    v_g2d, v_colors = torch.zeros(n, 6, dtype=dtype), torch.zeros(n, D, dtype=dtype)
    loss = torch.zeros((), dtype=dtype)
    skip = set((int(t), int(p)) for t, p in skip)
    for bt in pl["batches"]:
        ids, inside = bt["ids"], bt["inside"]
        leaves = [t[ids].requires_grad_(grads) for t in rec]  # [B, L, 2 / 3 / - / D]
        o, a = _blend_batch(bt, *leaves, dtype)
        g = torch.where(inside[:, :, None], G[bt["pixel"]].to(dtype), torch.zeros((), dtype=dtype))
        part = (o * g).sum()
        if A is not None:
            part = part + (a * torch.where(inside, A[bt["pixel"]].to(dtype), torch.zeros((), dtype=dtype))).sum()
        loss = loss + part.detach()
        out[bt["pixel"][inside]] = o.detach()[inside]
        alpha_img[bt["pixel"][inside]] = a.detach()[inside]
        if not grads:
            continue
        gm, gc, go, gcol = torch.autograd.grad(part, leaves)
        rows = torch.cat([gm, gc, go[:, :, None]], dim=2)
        real = torch.arange(ids.shape[1])[None, :] < bt["lens"][:, None]
        for t, p in skip:
            hit = torch.nonzero(bt["tiles"] == t).reshape(-1)
            if hit.numel():
                real[int(hit[0]), p] = False
        v_g2d.index_add_(0, ids[real], rows[real])
        v_colors.index_add_(0, ids[real], gcol[real])
    res = dict(out=out.reshape(H, W, D), alpha_img=alpha_img.reshape(H, W), loss=loss)
    if grads:
        res.update(v_g2d=v_g2d, v_colors=v_colors)
    return res


def oracle_front(orc, means, quats, scales, opacities, viewmat, K, W, H):
    """Records, lists and cut of the CPU oracle (pinhole, classic) for a test without a device: dict(means2d, conics, opacities,
    flatten_ids, tile_offsets, gid, pix, proj, plan)."""
    g = [rg.np_f32(t) for t in (means, quats, scales, opacities)]
    proj = orc.project(g[0], g[1], g[2], rg.np_f32(viewmat), rg.np_f32(K), W, H)
    bins = orc.bin_sort(proj, W, H)
    gid, pix, _, _ = orc.blend_pairs(proj, bins, g[3], W, H)
    return dict(means2d=torch.from_numpy(proj["means2d"]), conics=torch.from_numpy(proj["conics"]), opacities=torch.from_numpy(g[3]),
                flatten_ids=bins["flatten_ids"], tile_offsets=bins["tile_offsets"], gid=gid, pix=pix, proj=proj,
                plan=plan(bins["flatten_ids"], bins["tile_offsets"], gid, pix, W, H, g[0].shape[0]))


# ---- figures ---------------------------------------------------------------------------------------------------------------------
def row_error(got, truth):
    """The largest per-row error norm over max(|truth row|, 1e-3 x the largest row norm), in float64."""
    got, truth = got.detach().cpu().double(), truth.detach().cpu().double()
    num, den = (got - truth).norm(dim=1), truth.norm(dim=1)
    top = float(den.max())
    if top == 0.0:  # nothing to be relative to: any difference at all is an error of 1
        return float(float(num.max()) > 0.0)
    return float((num / den.clamp_min(1e-3 * top)).max())


def figures(v_g2d, v_colors, truth):
    """{(quantity, figure): value} of one side against the float64 truth: "fro" and "max" (raster_grad_ref.errors) of each of the
    six columns of v_g2d and of v_colors, "row" (row_error) of the mean, conic and opacity columns and of v_colors.  v_colors None
    (want_colors=False): the colour figures are left out."""
    out = {}
    for k, name in enumerate(COLUMNS):
        out[name, "fro"], out[name, "max"] = rg.errors(v_g2d[:, k], truth["v_g2d"][:, k])
    for name, sl in ROW_GROUPS:
        out[name, "row"] = row_error(v_g2d[:, sl], truth["v_g2d"][:, sl])
    if v_colors is not None:
        out["colors", "fro"], out["colors", "max"] = rg.errors(v_colors, truth["v_colors"])
        out["colors", "row"] = row_error(v_colors, truth["v_colors"])
    return out


def report(case, kernel, truth, floor32):
    """One dict per (quantity, figure): the float32 run's error (the floor), the kernel's, and their ratio (None over a floor of 0).
    kernel: (v_g2d, v_colors or None)."""
    f, k = figures(floor32["v_g2d"], floor32["v_colors"], truth), figures(kernel[0], kernel[1], truth)
    rows = []
    for key in k:
        rows.append(dict(case=case, quantity=key[0], figure=key[1], floor=f[key], kernel=k[key],
                         ratio=(k[key] / f[key]) if f[key] > 0.0 else None))
    return rows


def failures(rows, factor):
    """The rows that miss the rule: kernel error <= factor x the float32 floor, per quantity, per figure and per case."""
    return [r for r in rows if not r["kernel"] <= factor * r["floor"]]


def show(rows):
    for r in rows:
        ratio = "   -" if r["ratio"] is None else f"{r['ratio']:5.2f}"
        print(f"{r['case']:28s} {r['quantity']:8s} {r['figure']:4s} floor {r['floor']:.2e}   kernel {r['kernel']:.2e}   ratio {ratio}")
