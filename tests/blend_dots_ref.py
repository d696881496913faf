"""The dots form of the blend backward (k_render_dots_bwd, csrc/render_grad_wide.hip) restated in torch on the plan of
tests/blend_grad_ref.py, WITHOUT autograd: what the kernel computes, written out, so that the identity it rests on can be checked in
float64 against the differentiated blend.

For a (pixel p, record j) pair of a tile's list, with m_j = <c_j, vo_p>, fac_k = alpha_k T_k and ra_j = 1 / (1 - alpha_j):

    v_al_j = T_j m_j - ra_j B_j + T_final ra_j va_p,      B_j = sum over the records k behind j of fac_k m_k

    v_sigma = -(raw v_al) where the pair is valid and raw = o exp(-sigma) <= 0.999, else 0
    d / d(mx, my) = v_sigma (ca dx + cb dy, cb dx + cc dy),  d / d(ca, cb, cc) = v_sigma (dx^2 / 2, dx dy, dy^2 / 2),  d / d o = exp(-sigma) v_al

mutant (for the tests that show the comparison has teeth): "no-B" drops the B term, "alpha-for-fac" accumulates alpha_k m_k in B,
"no-va" drops the alpha map's term.
"""
import torch

import blend_grad_ref as bg


def v_g2d_dots(dtype, pl, means2d, conics, opacities, colors, v_out, v_alpha=None, mutant=None):
    W, H, n = pl["W"], pl["H"], pl["n"]
    m2d, con, opa, col = [torch.as_tensor(t).detach().cpu().to(dtype) for t in (means2d, conics, opacities, colors)]
    D = col.shape[1]
    G = torch.as_tensor(v_out).detach().cpu().reshape(H * W, D).to(dtype)
    A = torch.zeros(H * W, dtype=dtype) if v_alpha is None else torch.as_tensor(v_alpha).detach().cpu().reshape(H * W).to(dtype)
    zero = torch.zeros((), dtype=dtype)
    out = torch.zeros(n, 6, dtype=dtype)
    for bt in pl["batches"]:
        ids, mask, inside = bt["ids"], bt["mask"], bt["inside"]
        mx, my, ca, cb, cc, o = m2d[ids][..., 0], m2d[ids][..., 1], con[ids][..., 0], con[ids][..., 1], con[ids][..., 2], opa[ids]
        dx = mx[:, None, :] - (bt["px"].to(dtype) + 0.5)[:, :, None]
        dy = my[:, None, :] - (bt["py"].to(dtype) + 0.5)[:, :, None]
        sigma = 0.5 * (ca[:, None, :] * dx * dx + cc[:, None, :] * dy * dy) + cb[:, None, :] * dx * dy
        sigma = torch.where(mask, sigma, zero)
        vis = torch.exp(-sigma)
        raw = torch.where(mask, o[:, None, :] * vis, zero)
        alpha = torch.clamp(raw, max=bg.ALPHA_MAX)
        t_incl = torch.cumprod(1.0 - alpha, dim=2)
        T = torch.cat([torch.ones_like(t_incl[:, :, :1]), t_incl[:, :, :-1]], dim=2)
        T_final = t_incl[:, :, -1:]
        vo = torch.where(inside[:, :, None], G[bt["pixel"]], zero)          # [B, 256, D]
        va = torch.where(inside, A[bt["pixel"]], zero)[:, :, None]          # [B, 256, 1]
        m = torch.where(mask, torch.bmm(vo, col[ids].transpose(1, 2)), zero)  # [B, 256, L]
        w = (alpha if mutant == "alpha-for-fac" else alpha * T) * m
        B = w.flip(2).cumsum(dim=2).flip(2) - w                             # exclusive sum from behind
        ra = 1.0 / (1.0 - alpha)
        v_al = T * m
        if mutant != "no-B":
            v_al = v_al - ra * B
        if mutant != "no-va":
            v_al = v_al + T_final * ra * va
        moves = mask & (raw <= bg.ALPHA_MAX)
        v_sigma = torch.where(moves, -(raw * v_al), zero)
        rows = torch.stack([(v_sigma * (ca[:, None, :] * dx + cb[:, None, :] * dy)).sum(dim=1),
                            (v_sigma * (cb[:, None, :] * dx + cc[:, None, :] * dy)).sum(dim=1),
                            (0.5 * v_sigma * dx * dx).sum(dim=1), (v_sigma * dx * dy).sum(dim=1), (0.5 * v_sigma * dy * dy).sum(dim=1),
                            torch.where(moves, vis * v_al, zero).sum(dim=1)], dim=2)  # [B, L, 6]
        real = torch.arange(ids.shape[1])[None, :] < bt["lens"][:, None]
        out.index_add_(0, ids[real], rows[real])
    return out
