"""Per-view votes on the GPU (gwbp_vote_labels, gwbp_vote_projected, create_vote_field, mask3d_from_votes): every count must equal
the numpy restatement on the CPU oracle's pairs and projection exactly (counts are integers), and the two-class masks must equal
get_mask3d's voting loops run literally through the drop-in rasterization() and autograd."""
import numpy as np
import pytest
import torch

from util import scene_np, to_dev
from votes_ref import binary_votes, oracle_view, projection_votes

import gsbp_amd
from gsbp_amd import _lib, rasterization
from gsbp_amd import synthetic as syn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def t1(dev):
    cfg, sc = scene_np("T1")
    return cfg, sc, to_dev(sc, dev)


@pytest.fixture(scope="module")
def t1_pairs(t1, orc):
    cfg, sc, _ = t1
    h = [sc[k].numpy() for k in ("means", "quats", "scales", "opac")]
    return [oracle_view(orc, *h, sc["vms"][v].numpy(), sc["K"].numpy(), cfg.width, cfg.height) for v in range(cfg.n_views)]


def _gauss(g):
    return g["means"], g["quats"], g["scales"], g["opac"]


def _field(cfg, g, label_fn, K, method, **kw):
    C, n = gsbp_amd.create_vote_field(*_gauss(g), g["vms"], g["K"], cfg.width, cfg.height, label_fn, K, method=method, **kw)
    assert C.shape == (cfg.n_gaussians, K) and n.shape == (cfg.n_gaussians,) and C.dtype == n.dtype == torch.float32
    return C.cpu().numpy().astype(np.float64), n.cpu().numpy().astype(np.float64)


def _ref(cfg, pairs, maps, K, method, weights=None):
    C, n = np.zeros((cfg.n_gaussians, K)), np.zeros(cfg.n_gaussians)
    for v, (proj, gid, pix, w) in enumerate(pairs):
        L = maps[v].cpu().numpy()
        c = weights[v].float().cpu().numpy() if weights is not None else None
        Cv, nv = (binary_votes(gid, pix, w, L, K, cfg.n_gaussians, weights=c) if method == "binary"
                  else projection_votes(proj["means2d"], proj["radii"], L, K, weights=c))
        C += Cv
        n += nv
    return C, n


def _literal_masks(g, cfg, masks, method):
    """get_mask3d (affordance_transfer/demo_affordance_transfer.py) for one method, literally: zero colours with grad, per view
    loss = (render * mask).mean() and (render * ~mask).mean(), votes from colors.grad (binary: norm > 0; gradient: the norms);
    projection from meta["means2d"] / meta["gaussian_ids"] with np.round."""
    N = cfg.n_gaussians
    colors = torch.zeros(N, 3, device=g["means"].device, requires_grad=True)
    votes = torch.zeros(N, device=g["means"].device)
    for v, mask in enumerate(masks):
        m = mask.to(g["means"].device)
        out, _, meta = rasterization(*_gauss(g), colors, g["vms"][v][None], g["K"][None], width=cfg.width, height=cfg.height)
        (out[0] * m[..., None].float()).mean().backward(retain_graph=True)
        if method == "gradient":
            votes += colors.grad.norm(dim=1)
        elif method == "binary":
            votes += 1 * (colors.grad.norm(dim=1) > 0)
        else:
            xy = np.round(meta["means2d"].detach().cpu().numpy()).astype(int)
            inside = (xy[:, 0] >= 0) & (xy[:, 0] < cfg.width) & (xy[:, 1] >= 0) & (xy[:, 1] < cfg.height)
            xy = xy[inside]
            gids = meta["gaussian_ids"].detach().cpu().numpy()[inside]
            hit = mask.cpu().numpy()[xy[:, 1], xy[:, 0]]
            votes[torch.from_numpy(gids[~hit]).long().to(votes.device)] -= 1
            votes[torch.from_numpy(gids[hit]).long().to(votes.device)] += 1
        colors.grad.zero_()
        (out[0] * (~m)[..., None].float()).mean().backward()
        if method == "gradient":
            votes -= colors.grad.norm(dim=1)
        elif method == "binary":
            votes -= 1 * (colors.grad.norm(dim=1) > 0)
        colors.grad.zero_()
    return votes


def _masks(cfg, n_views=None):
    return [syn.make_label_map(cfg, v, 2) == 1 for v in range(n_views or cfg.n_views)]


@pytest.mark.parametrize("pipeline", [True, False])
def test_binary_k2_equals_pairs_and_get_mask3d(t1, t1_pairs, dev, pipeline):
    cfg, _, g = t1
    masks = _masks(cfg)
    C, n = _field(cfg, g, lambda v: masks[v].to(dev), 2, "binary", pipeline=pipeline)
    Cr, nr = _ref(cfg, t1_pairs, masks, 2, "binary")
    assert np.array_equal(C, Cr) and np.array_equal(n, nr) and n.max() == cfg.n_views
    m3, m3i = gsbp_amd.mask3d_from_votes(torch.from_numpy(C))
    votes = _literal_masks(g, cfg, masks, "binary").cpu()
    assert torch.equal(m3, votes > 0) and torch.equal(m3i, votes < 0) and m3.any() and m3i.any()


def test_projection_equals_get_mask3d_loop(t1, t1_pairs, dev):
    cfg, _, g = t1
    masks = _masks(cfg)
    C, n = _field(cfg, g, lambda v: masks[v].to(dev), 2, "projection")
    Cr, nr = _ref(cfg, t1_pairs, masks, 2, "projection")
    assert np.array_equal(C, Cr) and np.array_equal(n, nr) and n.sum() > 0
    votes = _literal_masks(g, cfg, masks, "projection").cpu().numpy()
    assert np.array_equal(C[:, 1] - C[:, 0], votes)
    m3, m3i = gsbp_amd.mask3d_from_votes(torch.from_numpy(C))
    assert np.array_equal(m3.numpy(), votes > 0) and np.array_equal(m3i.numpy(), votes < 0)


def test_projection_rounds_half_to_even(dev):
    """Centres placed exactly on x.5 (fx = fy = 1, cx = cy = 0, z = 1: u = x exactly) at even and odd integers and at both
    image edges: the votes are those of np.round on the drop-in's meta["means2d"]."""
    W, H = 40, 24
    xs = [-1.5, -0.5, 0.5, 1.5, 2.5, 3.5, 10.5, 11.5, 38.5, 39.5, 7.25, 7.75]
    ys = [-0.5, 0.5, 1.5, 4.5, 5.5, 22.5, 23.5]
    pts = torch.tensor([[x, y, 1.0] for x in xs for y in ys], dtype=torch.float32)
    N = pts.shape[0]
    means = pts.to(dev)
    quats = torch.tensor([[1.0, 0, 0, 0]] * N, device=dev)
    scales = torch.full((N, 3), 0.5, device=dev)
    opac = torch.full((N,), 0.9, device=dev)
    vm = torch.eye(4, device=dev)[None]
    K = torch.tensor([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]], device=dev)
    labels = (torch.arange(H)[:, None] * 7 + torch.arange(W)[None, :] * 3) % 5
    _, _, meta = rasterization(means, quats, scales, opac, torch.zeros(N, 3, device=dev), vm, K[None], width=W, height=H)
    m2d = meta["means2d"].cpu().numpy()
    assert np.array_equal(m2d, pts[meta["gaussian_ids"].cpu().long(), :2].numpy())  # the centres land exactly on the halves
    radii = np.zeros(N, np.int32)
    radii[meta["gaussian_ids"].cpu().numpy()] = 1
    full = np.zeros((N, 2), np.float32)
    full[meta["gaussian_ids"].cpu().numpy()] = m2d
    Cr, nr = projection_votes(full, radii, labels.numpy(), 5)
    C, n = gsbp_amd.create_vote_field(means, quats, scales, opac, vm, K, W, H, lambda v: labels.to(dev), 5, method="projection")
    assert np.array_equal(C.cpu().numpy(), Cr) and np.array_equal(n.cpu().numpy(), nr)
    # half to even: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4, -0.5 -> -0 (column 0), 39.5 -> 40 (outside)
    col = {x: int(np.round(np.float32(x))) for x in xs}
    assert col[0.5] == 0 and col[1.5] == 2 and col[2.5] == 2 and col[3.5] == 4 and col[10.5] == 10 and col[11.5] == 12
    voted = n.cpu().numpy().reshape(len(xs), len(ys))
    assert voted[xs.index(-0.5), ys.index(0.5)] == 1 and voted[xs.index(39.5), ys.index(0.5)] == 0
    assert voted[xs.index(-1.5)].sum() == 0 and voted[:, ys.index(23.5)].sum() == 0 and voted[:, ys.index(-0.5)].sum() > 0


def test_gradient_is_the_label_field_sums(t1, dev):
    cfg, _, g = t1
    masks = _masks(cfg)
    C, n = _field(cfg, g, lambda v: masks[v].to(dev), 2, "gradient")
    _, F, d, _ = gsbp_amd.create_label_field(*_gauss(g), g["vms"], g["K"], cfg.width, cfg.height, lambda v: masks[v].to(dev), 2,
                                             return_partials=True)
    F, d = F.cpu().numpy(), d.cpu().numpy()
    assert np.allclose(C, F, rtol=1e-5, atol=1e-9) and np.allclose(n, d, rtol=1e-5, atol=1e-9)
    votes = _literal_masks(g, cfg, masks, "gradient").cpu().numpy().astype(np.float64)
    diff = C[:, 1] - C[:, 0]
    none = (C[:, 1] + C[:, 0]) == 0  # Gaussians no view saw: 0 in both
    assert (votes[none] == 0).all() and (diff[none] == 0).all()
    tie = ~none & (np.abs(diff) <= 1e-5 * (C[:, 1] + C[:, 0]))  # (a near tie may take either sign under another summation order)
    assert np.array_equal(np.sign(diff)[~tie], np.sign(votes)[~tie]) and tie.sum() <= 2
    assert (np.sign(diff) != 0).sum() > 0


@pytest.mark.parametrize("K", [64, 1000])
@pytest.mark.parametrize("per_pixel", [False, True])
@pytest.mark.parametrize("method", ["binary", "projection"])
def test_many_classes_and_ignored_ids(t1, t1_pairs, dev, K, per_pixel, method):
    """Voronoi and per-pixel-random labels with ids -1 and >= K (ignored: they count in n and in no column); K = 1000 spans 32
    words of the bitset and many leader rounds per record; int16 and int64 maps."""
    cfg, _, g = t1
    maps = [syn.make_label_map(cfg, v, K + 4, per_pixel=per_pixel) - 2 for v in range(cfg.n_views)]
    for m in maps:  # (and bands of ignored ids whatever the random ids are)
        m[:5] = -1
        m[-5:] = K + 7
    dt = torch.int16 if per_pixel else torch.int64
    C, n = _field(cfg, g, lambda v: maps[v].to(dt).to(dev), K, method)
    Cr, nr = _ref(cfg, t1_pairs, maps, K, method)
    assert np.array_equal(C, Cr) and np.array_equal(n, nr)
    assert (n > C.sum(1)).any()  # Gaussians that voted in some view for ignored ids only


def test_pipeline_equals_serial_on_overlapping_views(dev, orc):
    """Nine overlapping views through three workspaces (commits of different views may be in flight together) equal one stream."""
    cfg, sc = scene_np("T1", n_views=9)
    g = to_dev(sc, dev)
    maps = [syn.make_label_map(cfg, v, 6) for v in range(cfg.n_views)]
    C1, n1 = _field(cfg, g, lambda v: maps[v].to(dev), 6, "binary", pipeline=3)
    C0, n0 = _field(cfg, g, lambda v: maps[v].to(dev), 6, "binary", pipeline=False)
    assert np.array_equal(C1, C0) and np.array_equal(n1, n0) and n0.max() >= 3
    h = [sc[k].numpy() for k in ("means", "quats", "scales", "opac")]
    pairs = [oracle_view(orc, *h, sc["vms"][v].numpy(), sc["K"].numpy(), cfg.width, cfg.height) for v in range(cfg.n_views)]
    Cr, nr = _ref(cfg, pairs, maps, 6, "binary")
    assert np.array_equal(C0, Cr) and np.array_equal(n0, nr)


def test_reused_engine(t1, dev):
    cfg, _, g = t1
    maps = [syn.make_label_map(cfg, v, 70) for v in range(cfg.n_views)]
    feats = [syn.make_feature_map(cfg, v) for v in range(cfg.n_views)]

    def lab(v):
        return maps[v].to(dev)

    def feat(v):
        return feats[v].to(dev)
    args = (*_gauss(g), g["vms"], g["K"], cfg.width, cfg.height)
    eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev, tight_binning=True)
    a = _field(cfg, g, lab, 70, "binary", engine=eng)
    b = _field(cfg, g, lab, 70, "binary", engine=eng)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    P = gsbp_amd.create_label_field(*args, lab, 70, engine=eng).cpu()
    c = _field(cfg, g, lab, 70, "projection", engine=eng)
    Fe = gsbp_amd.create_feature_field(*args, feat, cfg.feat_dim, engine=eng).cpu()
    d2 = _field(cfg, g, lab, 70, "binary", engine=eng, pipeline=False)
    P0 = gsbp_amd.create_label_field(*args, lab, 70).cpu()
    Fe0 = gsbp_amd.create_feature_field(*args, feat, cfg.feat_dim).cpu()
    c0 = _field(cfg, g, lab, 70, "projection")
    assert torch.allclose(P, P0, rtol=1e-5, atol=1e-6) and torch.allclose(Fe, Fe0, rtol=1e-4, atol=1e-5)
    assert np.array_equal(c[0], c0[0]) and np.array_equal(c[1], c0[1])
    assert np.array_equal(d2[0], a[0]) and np.array_equal(d2[1], a[1])


@pytest.mark.parametrize("method", ["binary", "projection"])
def test_nearest_upsampled_labels(t1, dev, method):
    cfg, _, g = t1
    lo = [syn.make_label_map(cfg, v, 9, size=(17, 25)) - 1 for v in range(cfg.n_views)]
    up = [torch.nn.functional.interpolate(m[None, None].float(), size=(cfg.height, cfg.width), mode="nearest")[0, 0].to(torch.int32)
          for m in lo]
    a = _field(cfg, g, lambda v: lo[v].to(dev), 8, method, upsample="nearest")
    b = _field(cfg, g, lambda v: up[v].to(dev), 8, method)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[1].sum() > 0


@pytest.mark.parametrize("method", ["binary", "projection"])
def test_pixel_weights(t1, t1_pairs, dev, method):
    """Weights in (0, 1] count as no weights; a pixel of weight 0 casts no vote (not in n either): C equals the vote of the map
    whose weight-0 pixels are ignored labels, n the reference on the weighted pairs."""
    cfg, _, g = t1
    maps = [syn.make_label_map(cfg, v, 4) for v in range(cfg.n_views)]
    conf = [syn.make_pixel_weights(cfg, v, kind="confidence").clamp(min=1e-3, max=1.0) for v in range(cfg.n_views)]
    mask = [syn.make_pixel_weights(cfg, v, kind="mask") for v in range(cfg.n_views)]
    assert all(float(c.min()) > 0 for c in conf) and all(bool((m == 0).any()) for m in mask)
    plain = _field(cfg, g, lambda v: maps[v].to(dev), 4, method)
    wc = _field(cfg, g, lambda v: maps[v].to(dev), 4, method, pixel_weight_fn=lambda v: conf[v].to(dev))
    assert np.array_equal(plain[0], wc[0]) and np.array_equal(plain[1], wc[1])
    wm = _field(cfg, g, lambda v: maps[v].to(dev), 4, method, pixel_weight_fn=lambda v: mask[v].to(dev))
    Cr, nr = _ref(cfg, t1_pairs, maps, 4, method, weights=mask)
    assert np.array_equal(wm[0], Cr) and np.array_equal(wm[1], nr) and nr.sum() < plain[1].sum()
    ignored = [torch.where(mask[v] != 0, maps[v], -1) for v in range(cfg.n_views)]
    ig = _field(cfg, g, lambda v: ignored[v].to(dev), 4, method)
    assert np.array_equal(wm[0], ig[0])


@pytest.mark.parametrize("method", ["binary", "projection"])
@pytest.mark.parametrize("pipeline", [True, False])
def test_render_fed_labels(t1, dev, method, pipeline):
    cfg, _, g = t1
    coeffs = syn.make_sh_coeffs(cfg, 3).to(dev)
    seen = {}

    def label_fn(v, image):
        with torch.no_grad():
            ref, _, _ = rasterization(*_gauss(g), coeffs, g["vms"][v][None], g["K"][None], width=cfg.width, height=cfg.height,
                                      sh_degree=3, want_meta=False)
        seen[v] = torch.equal(image, ref[0])
        return (image[..., 0] > image[..., 1]).to(torch.uint8)
    C, n = _field(cfg, g, label_fn, 2, method, render_colors=coeffs, sh_degree=3, pipeline=pipeline)
    assert sorted(seen) == list(range(cfg.n_views)) and all(seen.values())
    imgs = [rasterization(*_gauss(g), coeffs, g["vms"][v][None], g["K"][None], width=cfg.width, height=cfg.height,
                          sh_degree=3, want_meta=False)[0][0] for v in range(cfg.n_views)]
    lab = [(im[..., 0] > im[..., 1]).to(torch.uint8) for im in imgs]
    C2, n2 = _field(cfg, g, lambda v: lab[v], 2, method)
    assert np.array_equal(C, C2) and np.array_equal(n, n2) and n.sum() > 0


def test_binary_vote_after_token_blend_sets_mismatch_and_adds_nothing(t1, dev):
    cfg, _, g = t1
    eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev)
    view = eng.view(g["vms"][0], g["K"], cfg.width, cfg.height)
    eng.project(view, *_gauss(g))
    eng.bin_sort(view)
    eng.blend_tokens(view, 8, 12)
    L = syn.make_label_map(cfg, 0, 3).to(dev)
    C = torch.zeros(cfg.n_gaussians, 3, device=dev)
    n = torch.zeros(cfg.n_gaussians, device=dev)
    with pytest.raises(gsbp_amd.GwbpError):
        eng.vote_labels(view, L, C, n, 3)  # the Engine refuses first
    seen = eng._vote_seen(3)
    import ctypes
    eng._call("gwbp_vote_labels", *eng._args(), ctypes.byref(view), _lib.ptr(L), _lib.LABEL_I32, L.stride(0), L.stride(1), None,
              None, 3, _lib.ptr(seen), _lib.ptr(C), C.stride(0), _lib.ptr(n), eng._stream())
    st = eng.stats()
    assert st["overflow"] & 4
    assert int(C.count_nonzero()) == 0 and int(n.count_nonzero()) == 0 and int(seen.count_nonzero()) == 0


def test_engine_argument_errors(t1, dev):
    cfg, _, g = t1
    eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev)
    view = eng.view(g["vms"][0], g["K"], cfg.width, cfg.height)
    L = syn.make_label_map(cfg, 0, 3).to(dev)
    C = torch.zeros(cfg.n_gaussians, 3, device=dev)
    n = torch.zeros(cfg.n_gaussians, device=dev)
    for bad in (dict(labels=L.float()), dict(labels=L.cpu()), dict(labels=L[:5]), dict(C=C[:, :2]), dict(C=C.double()),
                dict(n=n[:5]), dict(num_classes=0), dict(upsample="bilinear")):
        kw = dict(labels=L, C=C, n=n, num_classes=3) | bad
        for fn in (eng.vote_labels, eng.vote_projected):
            with pytest.raises(gsbp_amd.GwbpError):
                fn(view, kw["labels"], kw["C"], kw["n"], kw["num_classes"], upsample=kw.get("upsample"))
    with pytest.raises(gsbp_amd.GwbpError):
        eng.vote_projected(view, L, C, n, 3, pixel_weights=torch.ones(3, 3, device=dev))
