"""TEST SUPPORT: the depth losses (csrc/depth_math.h, csrc/depth_loss.hip) restated, no GPU.

  * point_terms32 / map_terms32: the header's text in numpy float32, operation by operation -- what the host build of the header and
    the kernels must give bit for bit.  `mutant=` swaps in one of the wrong readings the comparison has to catch.
  * point_terms64 / map_terms64: the same formulas in float64 on the same float32 inputs -- the truth.
  * literal_point_loss: the reference trainer's lines as it writes them in torch (ED division, grid_sample(align_corners=True), where,
    l1_loss), evaluated in whatever dtype it is handed.
  * the cases the tests share (make_image, make_points, make_depth_map).
"""
import numpy as np

F = np.float32
AMIN = F(1e-10)  # the clamp of the alpha map, as the float32 constant the header holds
MUTANTS = ("pixel_centre", "clamped_padding", "eps_division", "no_q2", "no_alpha_rule")
CHAIN = 28  # roundings on the way from the inputs to one share of v_alpha (test_gpu_depth_loss.py derives it)


# ---- the point term -------------------------------------------------------------------------------------------------------------------
def _corners(H, W, x, y, dt, mutant):
    """Per point and corner (00, 01, 10, 11): in-image flag, row, column (clipped to the image where the flag is off)."""
    x0, y0 = np.floor(x), np.floor(y)
    cols = np.stack([x0, x0 + dt(1), x0, x0 + dt(1)], axis=1)
    rows = np.stack([y0, y0, y0 + dt(1), y0 + dt(1)], axis=1)
    inside = (rows >= 0) & (rows < H) & (cols >= 0) & (cols < W)
    r = np.clip(np.nan_to_num(rows), 0, H - 1).astype(np.int64)
    c = np.clip(np.nan_to_num(cols), 0, W - 1).astype(np.int64)
    if mutant == "clamped_padding":
        inside = np.ones_like(inside)
    return x0, y0, inside, r, c


def _point_terms(A, a, points, g, c, dt, mutant=None):
    """The chain of depth_math.h in the dtype dt.  A, a: [H, W]; points [M, 2]; g [M]; c: the backward's scalar (upstream * scale / M).
    Returns a dict: d, q, r, t [M]; inside, row, col [M, 4]; v_e, v_A, v_a [M, 4] (zeros where the corner is outside)."""
    assert mutant is None or mutant in MUTANTS
    A, a, g, c = np.asarray(A, dt), np.asarray(a, dt), np.asarray(g, dt), dt(c)
    H, W = A.shape
    x, y = np.asarray(points[:, 0], dt), np.asarray(points[:, 1], dt)
    if mutant == "pixel_centre":
        x, y = x - dt(0.5), y - dt(0.5)
    amin, one = dt(AMIN), dt(1)
    x0, y0, inside, row, col = _corners(H, W, x, y, dt, mutant)
    with np.errstate(all="ignore"):
        Ak, ak = A[row, col], a[row, col]
        am = np.where(ak < amin, amin, ak)
        e = np.where(inside, Ak / am, dt(0))
        fx, fy = x - x0, y - y0
        gx, gy = one - fx, one - fy
        top = gx * e[:, 0] + fx * e[:, 1]
        bot = gx * e[:, 2] + fx * e[:, 3]
        d = gy * top + fy * bot
        if mutant == "eps_division":
            q = one / (d + dt(1e-10))
        else:
            q = np.where(d > 0, one / np.where(d > 0, d, one), dt(0))
        r = q - one / g
        t = np.abs(r)
        sgn = np.where(r > 0, one, np.where(r < 0, -one, dt(0)))
        q2 = q if mutant == "no_q2" else q * q
        v_d = np.where(d > 0, -(sgn * (q2 * c)), dt(0)) if mutant != "eps_division" else -(sgn * (q2 * c))
        w = np.stack([gy * gx, gy * fx, fy * gx, fy * fx], axis=1)
        v_e = w * v_d[:, None]
        v_A = np.where(inside, v_e / am, dt(0))
        passes = np.ones_like(inside) if mutant == "no_alpha_rule" else ak >= amin
        v_a = np.where(inside & passes, -((v_e * Ak) / np.where(passes & (ak != 0), ak * ak, one)), dt(0))
    return dict(d=d.astype(dt), q=q.astype(dt), r=r.astype(dt), t=t.astype(dt), inside=inside, row=row, col=col,
                v_e=v_e.astype(dt), v_A=v_A.astype(dt), v_a=v_a.astype(dt))


def point_terms32(A, a, points, g, c=1.0, mutant=None):
    return _point_terms(A, a, points, g, c, F, mutant)


def point_terms64(A, a, points, g, c=1.0, mutant=None):
    return _point_terms(A, a, points, g, c, np.float64, mutant)


def scale_over_m(scale, M):
    """(float)(scale / M) as the launcher forms it: float64, rounded once."""
    return F(np.float64(F(scale)) / np.float64(M))


def point_loss64(terms, scale, M):
    """scale (sum t) / M in float64 from per-point terms; 0 for M = 0."""
    return 0.0 if M == 0 else float(np.float64(F(scale)) * np.sum(terms["t"].astype(np.float64)) / M)


def scatter_maps(terms, H, W):
    """What the shares of a term dict sum to per pixel, in float64: (v_A [H, W], v_a [H, W], sum |v_A|, sum |v_a|, the number of
    non-zero shares of v_A per pixel, ... of v_a)."""
    out = [np.zeros((H, W)) for _ in range(4)] + [np.zeros((H, W), np.int64) for _ in range(2)]
    idx = (terms["row"][terms["inside"]], terms["col"][terms["inside"]])
    vA, va = terms["v_A"][terms["inside"]].astype(np.float64), terms["v_a"][terms["inside"]].astype(np.float64)
    np.add.at(out[0], idx, vA), np.add.at(out[1], idx, va)
    np.add.at(out[2], idx, np.abs(vA)), np.add.at(out[3], idx, np.abs(va))
    np.add.at(out[4], idx, (vA != 0).astype(np.int64)), np.add.at(out[5], idx, (va != 0).astype(np.int64))
    return out


def grad_bound(count, total_abs):
    """(count + CHAIN) 2^-24 sum |shares| per pixel: each share carries at most CHAIN roundings, and the `count` float32 adds that
    gather them one more each on a partial sum that is at most sum |shares|."""
    return (count + CHAIN) * 2.0 ** -24 * total_abs


# ---- the map term ---------------------------------------------------------------------------------------------------------------------
def _map_terms(A, a, g, w, kind, c, dt):
    """Per pixel: valid, e, t (0 where invalid), v_A, v_a; c = upstream * scale / sum w."""
    A, a, g = np.asarray(A, dt), np.asarray(a, dt), np.asarray(g, dt)
    w = np.ones_like(g) if w is None else np.asarray(w, dt)
    amin, one, c = dt(AMIN), dt(1), dt(c)
    with np.errstate(all="ignore"):
        valid = (g > 0) & (w > 0)
        am = np.where(a < amin, amin, a)
        e = A / am
        q = np.where(e > 0, one / np.where(e > 0, e, one), dt(0))
        gs = np.where(valid, g, one)
        r = (e - gs) if kind == "depth" else (q - one / gs)
        t = np.where(valid, np.abs(r), dt(0))
        sgn = np.where(r > 0, one, np.where(r < 0, -one, dt(0)))
        wc = w * c
        v_e = sgn * wc if kind == "depth" else -(sgn * ((q * q) * wc))
        v_e = np.where(valid & (e > 0), v_e, dt(0))
        v_A = np.where(valid, v_e / am, dt(0))  # (a pixel that is not valid is not evaluated: +0, whatever the formula's zero)
        v_a = np.where(valid & (a >= amin), -((v_e * A) / np.where(a >= amin, a * a, one)), dt(0))
    return dict(valid=valid, e=e.astype(dt), t=t.astype(dt), w=np.where(valid, w, dt(0)).astype(dt), v_A=v_A.astype(dt), v_a=v_a.astype(dt))


def map_terms32(A, a, g, w=None, kind="disparity", c=1.0):
    return _map_terms(A, a, g, w, kind, c, F)


def map_terms64(A, a, g, w=None, kind="disparity", c=1.0):
    return _map_terms(A, a, g, w, kind, c, np.float64)


def map_sums64(terms):
    return (float(np.sum(terms["w"].astype(np.float64) * terms["t"].astype(np.float64))), float(np.sum(terms["w"].astype(np.float64))))


def map_loss64(terms, scale):
    swt, sw = map_sums64(terms)
    return float(np.float64(F(scale)) * swt / sw) if sw > 0 else 0.0


def map_c(upstream, scale, sw):
    """(float)(upstream * scale / sum w), float64 rounded once; 0 without a valid pixel."""
    return F(np.float64(F(upstream)) * np.float64(F(scale)) / sw) if sw > 0 else F(0)


# ---- the reference trainer's lines, literally ---------------------------------------------------------------------------------------------
def literal_point_loss(render, alpha, points, depths_gt, channel=-1, scale=1.0):
    """simple_trainer's depth term on torch tensors of any float dtype and device: render [H, W, D'] of an accumulated-depth mode, alpha
    [H, W].  Returns (loss, sampled depths [M]).  The clamp is the float32 constant the kernels hold, so that a float64 evaluation
    differs from the restatement by rounding alone."""
    import torch
    import torch.nn.functional as Fn
    height, width = render.shape[:2]
    depths = (render[..., channel] / alpha.clamp_min(float(AMIN)))[None, :, :, None]  # the ED render, [1, H, W, 1]
    pts = points[None]                                                                  # [1, M, 2]
    pts = torch.stack([pts[:, :, 0] / (width - 1) * 2 - 1, pts[:, :, 1] / (height - 1) * 2 - 1], dim=-1)  # normalize to [-1, 1]
    grid = pts.unsqueeze(2)                                                             # [1, M, 1, 2]
    depths = Fn.grid_sample(depths.permute(0, 3, 1, 2), grid, align_corners=True)       # [1, 1, M, 1]
    depths = depths.squeeze(3).squeeze(1)                                               # [1, M]
    disp = torch.where(depths > 0.0, 1.0 / depths, torch.zeros_like(depths))
    disp_gt = 1.0 / depths_gt[None]
    return Fn.l1_loss(disp, disp_gt) * scale, depths[0]


# ---- the cases --------------------------------------------------------------------------------------------------------------------------
def make_image(H=13, W=19, Dp=4, ch=3, seed=0):
    """(render [H, W, Dp], alpha [H, W]) float32: depths in [0.5, 8] under alphas in (0.2, 1], other channels noise, with a block of
    empty pixels (a = 0, A = 0) at the top right, a few pixels with 0 < a < 1e-10, and a few with a = 1 exactly."""
    rng = np.random.default_rng(seed)
    alpha = rng.uniform(0.2, 1.0, (H, W)).astype(F)
    depth = rng.uniform(0.5, 8.0, (H, W)).astype(F)
    render = rng.standard_normal((H, W, Dp)).astype(F)
    alpha[2, 3] = alpha[7, 11] = alpha[H - 1, W - 1] = F(1.0)
    A = (depth * alpha).astype(F)
    alpha[0:4, W - 5:W] = 0.0
    A[0:4, W - 5:W] = 0.0
    for (r, c), a_small, e in (((5, 2), 3e-11, 2.5), ((9, 14), 7e-12, 0.75)):  # below the clamp: e = A / 1e-10
        alpha[r, c] = F(a_small)
        A[r, c] = F(e) * AMIN
    render[..., ch] = A
    return render, alpha


def make_points(M, H=13, W=19, seed=0):
    """(points [M, 2], depths [M]) float32.  The first entries are the listed edge cases, in this order, as far as M reaches: (0, 0);
    integer coordinates; x in (W - 1, W); y in (H - 1, H); both; eight points inside one cell (shared corners); points over the empty
    block (all four corners a = 0: d = 0), on its edge, over the pixels below the clamp and over a = 1; the rest seeded uniform.
    The true depths span six decades."""
    rng = np.random.default_rng(1000 + seed)
    fixed = [(0.0, 0.0), (4.0, 6.0), (W - 1.0, H - 1.0), (W - 0.25, 3.5), (2.5, H - 0.5), (W - 0.75, H - 0.125)]
    fixed += [(8.0 + u, 6.0 + v) for u, v in ((0.1, 0.1), (0.9, 0.2), (0.5, 0.5), (0.25, 0.75), (0.7, 0.9), (0.05, 0.95), (0.6, 0.3),
                                              (0.33, 0.66))]
    fixed += [(W - 3.5, 1.5), (W - 2.25, 0.75), (W - 5.5, 2.5), (W - 4.5, 3.5), (1.5, 4.5), (2.0, 5.0), (13.5, 8.5), (14.0, 9.0),
              (3.0, 2.0), (10.5, 6.5), (11.0, 7.0)]
    pts = np.array(fixed[:M], F).reshape(-1, 2)
    if M > len(fixed):
        more = rng.uniform(0.0, 1.0, (M - len(fixed), 2)) * np.array([W, H])
        pts = np.concatenate([pts, more.astype(F)], axis=0)
        pts[:, 0] = np.minimum(pts[:, 0], np.nextafter(F(W), F(0)))
        pts[:, 1] = np.minimum(pts[:, 1], np.nextafter(F(H), F(0)))
    g = (10.0 ** rng.uniform(-3.0, 3.0, M)).astype(F)
    return pts.astype(F), g


def make_depth_map(H=13, W=19, seed=0, all_invalid=False):
    """(depth map [H, W], weights [H, W]) float32: a quarter of the map invalid (0 or negative), a fifth of the weights 0."""
    rng = np.random.default_rng(2000 + seed)
    g = rng.uniform(0.3, 9.0, (H, W)).astype(F)
    g[rng.uniform(size=(H, W)) < 0.25] = 0.0
    g[1, 1] = F(-2.0)
    w = rng.uniform(0.1, 2.0, (H, W)).astype(F)
    w[rng.uniform(size=(H, W)) < 0.2] = 0.0
    if all_invalid:
        g[:] = 0.0
    return g, w
