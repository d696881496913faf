"""Prompt segmentation on the GPU: gwbp_prompt_scores against the float64 reference within its rounding bound, the masks on every
decided row, storage and torch semantics; gwbp_probe_pixels bit for bit against the full render; the 2-D mask against the literal
D-channel form; a click session end to end."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gsbp_amd
from gsbp_amd import segment as seg
from gsbp_amd import synthetic as syn
from gsbp_amd.rasterization import get_engine

import segment_ref as ref
from test_segment_cpu import pixel_margins

pytestmark = pytest.mark.gpu

CASE_IDS = [f"N{c[0]}-D{c[1]}-P{c[2]}-pos{c[3]}" for c in ref.CASES]
EDGES = [(n, d, p, 1) for n in (1, 63, 4097) for d, p in ((1, 2), (3, 3), (30, 17), (1024, 32))]


def _check_scores(dev, case, normalize):
    x, t = ref.make_case(*case)
    got = gsbp_amd.prompt_scores(torch.from_numpy(x).to(dev), torch.from_numpy(t).to(dev), normalize=normalize).cpu().numpy()
    s, b = ref.scores(x, t, normalize), ref.bound(x, t, normalize)
    err = np.abs(got.astype(np.float64) - s)
    print(f"{case} normalize={normalize}: max err / bound = {float((err / np.maximum(b, 1e-300)).max()):.4f}")
    assert got.shape == s.shape and np.all(err <= b)


# ---- 6. scores --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("case", ref.CASES, ids=CASE_IDS)
def test_scores_are_within_the_rounding_bound(dev, case, normalize):
    _check_scores(dev, case, normalize)


@pytest.mark.parametrize("case", EDGES, ids=[f"N{c[0]}-D{c[1]}-P{c[2]}" for c in EDGES])
def test_scores_at_edge_sizes(dev, case):
    _check_scores(dev, case, True)
    _check_scores(dev, case, False)


# ---- 7. masks ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("case", ref.CASES, ids=CASE_IDS)
def test_mask_equals_the_reference_on_every_decided_row(dev, case, normalize):
    n, d, p, n_pos = case
    x, t = ref.make_case(*case)
    xd, td = torch.from_numpy(x).to(dev), torch.from_numpy(t).to(dev)
    s, b = ref.scores(x, t, normalize), ref.bound(x, t, normalize)
    thr = ref.threshold_of(s)
    for name, tt, ss, bb, th in (("plain", td, s, b, None), ("threshold", td, s, b, thr),
                                 ("no negatives", td[:n_pos], s[:, :n_pos], b[:, :n_pos], thr)):
        got = gsbp_amd.prompt_mask(xd, tt, n_pos, threshold=th, normalize=normalize).cpu().numpy()
        want, dec = ref.mask_of(ss, n_pos, th), ref.decided(ss, bb, n_pos, th)
        differ = got != want
        print(f"{case} normalize={normalize} {name}: {int((~dec).sum())} undecided rows, {int((differ & ~dec).sum())} of them differ; "
              f"{int((differ & dec).sum())} decided rows differ")
        assert got.dtype == bool and not (differ & dec).any()
        assert (~dec).mean() <= 0.01


# ---- 8. storage -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(4097, 30, 17, 3), (1000, 512, 4, 1), (777, 1028, 32, 5)], ids=["D30", "D512", "D1028"])
def test_storage_and_position_do_not_change_a_bit(dev, case):
    n, d, p, n_pos = case
    x, t = ref.make_case(*case)
    xd, td = torch.from_numpy(x).to(dev), torch.from_numpy(t).to(dev)
    base = gsbp_amd.prompt_scores(xd, td)
    base_mask = gsbp_amd.prompt_mask(xd, td, n_pos)
    # padded rows, NaN in the padding (16-B aligned rows when d + 4 is a multiple of 4, element-wise otherwise)
    for pad in (4, 5):
        wide = torch.full((n, d + pad), float("nan"), device=dev)
        wide[:, :d] = xd
        view = wide[:, :d]
        assert not view.is_contiguous() or n == 1
        assert torch.equal(gsbp_amd.prompt_scores(view, td), base) and torch.equal(gsbp_amd.prompt_mask(view, td, n_pos), base_mask)
    # a column slice at an odd offset
    wide = torch.full((n, d + 7), float("nan"), device=dev)
    wide[:, 3:3 + d] = xd
    assert torch.equal(gsbp_amd.prompt_scores(wide[:, 3:3 + d], td), base)
    assert torch.equal(gsbp_amd.prompt_scores(wide[:, 3:3 + d], td, normalize=False), gsbp_amd.prompt_scores(xd, td, normalize=False))
    # permuted rows: a row's scores do not depend on where it is, nor on how many rows there are
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(1)).to(dev)
    assert torch.equal(gsbp_amd.prompt_scores(xd[perm], td), base[perm])
    assert torch.equal(gsbp_amd.prompt_mask(xd[perm], td, n_pos), base_mask[perm])
    assert torch.equal(gsbp_amd.prompt_scores(xd[:131], td), base[:131])
    # ... nor on the other prompts
    assert torch.equal(gsbp_amd.prompt_scores(xd, td[:2]), base[:, :2])
    # twice the same
    assert torch.equal(gsbp_amd.prompt_scores(xd, td), base)


# ---- 9. torch semantics -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [True, False])
def test_zero_rows_nan_rows_and_agreement_of_mask_and_scores(dev, normalize):
    x, t = ref.make_case(600, 40, 6, 2)
    x[5] = 0.0
    x[9, 3] = np.nan
    x[11] = x[10]
    xd, td = torch.from_numpy(x).to(dev), torch.from_numpy(t).to(dev)
    thr = 0.1
    mask_u8, scores = seg._query(xd, td, 2, thr, normalize, True, True)   # both outputs of ONE call
    mask = mask_u8.bool()
    assert torch.equal(scores[5], torch.zeros(6, device=dev)) and not bool(mask[5])
    assert bool(torch.isnan(scores[9]).all()) and not bool(mask[9])
    assert not bool(gsbp_amd.prompt_mask(xd, td, 2, normalize=normalize)[9])
    assert torch.equal(scores[10], scores[11])
    assert torch.equal(mask, seg.mask_from_scores(scores, 2, thr))
    assert torch.equal(gsbp_amd.prompt_mask(xd, td, 2, normalize=normalize), seg.mask_from_scores(scores, 2))
    assert torch.equal(gsbp_amd.prompt_mask(xd, td[:2], 2, threshold=thr, normalize=normalize),
                       seg.mask_from_scores(scores[:, :2], 2, thr))
    # a NaN among the NEGATIVE scores loses as well (torch.max propagates it)
    tn = td.clone()
    tn[4, 0] = float("nan")
    assert not bool(gsbp_amd.prompt_mask(xd, tn, 2, normalize=normalize).any())
    with pytest.raises(gsbp_amd.GwbpError):
        gsbp_amd.prompt_mask(xd, td, 6)
    if normalize:
        want = F.normalize(xd[:5], dim=1) @ td.T
        assert torch.allclose(scores[:5], want, atol=1e-5)


# ---- 10. the probe ----------------------------------------------------------------------------------------------------------------
def _scene(cfg, dev):
    return tuple(t.to(dev) for t in syn.activate(syn.make_scene(cfg)))


def _probe_pixels_of(cfg, alpha_map):
    g = torch.Generator().manual_seed(4)
    xs, ys = torch.randint(0, cfg.width, (64,), generator=g), torch.randint(0, cfg.height, (64,), generator=g)
    xy = torch.stack([xs, ys], dim=1).tolist()
    xy += [[0, 0], [cfg.width - 1, 0], [0, cfg.height - 1], [cfg.width - 1, cfg.height - 1]]
    bare = torch.nonzero(alpha_map == 0)
    assert bare.numel() > 0, "the scene leaves no pixel uncovered"
    xy.append([int(bare[0, 1]), int(bare[0, 0])])
    return xy, xy + [[cfg.width, 3], [-1, 5]]   # inside, inside + two pixels outside the image


@pytest.mark.parametrize("kw", [{}, {"camera_model": "fisheye"}, {"rasterize_mode": "antialiased"}], ids=["pinhole", "fisheye", "aa"])
@pytest.mark.parametrize("D", [16, 64, 512, 1028])
def test_probe_equals_the_full_render_bit_for_bit(dev, D, kw):
    cfg = syn.CONFIGS["T1"]
    means, quats, scales, opac = _scene(cfg, dev)
    n_keep = 1500                                                    # a sparser scene: some pixels stay uncovered
    means, quats, scales, opac = (t[-n_keep:].contiguous() for t in (means, quats, scales * 0.6, opac))
    K, vm = syn.intrinsics(cfg).to(dev), syn.make_cameras(cfg).to(dev)[0]
    feats = torch.randn(n_keep, D, generator=torch.Generator().manual_seed(D)).to(dev)
    with torch.no_grad():
        full, alpha, _ = gsbp_amd.rasterization(means, quats, scales, opac, feats, vm[None], K[None], cfg.width, cfg.height,
                                                render_mode="RGB+D", want_meta=False, **kw)
    full, alpha = full[0], alpha[0, ..., 0]
    inside, everything = _probe_pixels_of(cfg, alpha)
    eng = get_engine(dev, n_keep, cfg.width, cfg.height)
    gen = eng.generation
    got, depth, a = gsbp_amd.probe_pixels(means, quats, scales, opac, feats, vm, K, cfg.width, cfg.height, everything, **kw)
    assert eng.generation == gen, "the probe re-projected a view the workspace already held"
    idx = torch.tensor(inside, device=dev)
    want = full[idx[:, 1], idx[:, 0]]
    m = len(inside)
    assert got.shape == (m + 2, D) and depth.shape == (m + 2,) and a.shape == (m + 2,)
    assert torch.equal(got[:m], want[:, :D]) and torch.equal(depth[:m], want[:, D]) and torch.equal(a[:m], alpha[idx[:, 1], idx[:, 0]])
    assert int((a[:64] > 0).sum()) >= 8, "the seeded pixels hit nothing"
    assert not bool(got[m - 1].any()) and float(depth[m - 1]) == 0.0 and float(a[m - 1]) == 0.0     # the uncovered pixel
    assert not bool(got[m:].any()) and not bool(depth[m:].any()) and not bool(a[m:].any())         # outside the image
    # a padded field is probed in place, with the same bits
    wide = torch.full((n_keep, D + 5), float("nan"), device=dev)
    wide[:, :D] = feats
    again = gsbp_amd.probe_pixels(means, quats, scales, opac, wide[:, :D], vm, K, cfg.width, cfg.height, everything, **kw)
    assert torch.equal(again[0], got) and torch.equal(again[1], depth) and torch.equal(again[2], a)
    # a probe of a view the workspace does not hold projects it (and then again does not)
    vm2 = syn.make_cameras(cfg).to(dev)[1]
    gsbp_amd.probe_pixels(means, quats, scales, opac, feats, vm2, K, cfg.width, cfg.height, [[10, 10]], **kw)
    assert eng.generation == gen + 1
    gsbp_amd.probe_pixels(means, quats, scales, opac, feats, vm2, K, cfg.width, cfg.height, [[11, 10]], **kw)
    assert eng.generation == gen + 1


# ---- 11. the 2-D mask -------------------------------------------------------------------------------------------------------------
def test_rendered_mask_equals_the_literal_form_on_every_decided_pixel(dev):
    scene = ref.two_blob_scene(n_per=60)
    rng = np.random.default_rng(5)
    prompts = (scene["feats"][[0, 60]] + 0.02 * rng.standard_normal((2, scene["feats"].shape[1]))).astype(np.float32)
    margin, slack, covered, want = pixel_margins(scene, prompts, 1)
    W, H = scene["width"], scene["height"]
    t = {k: torch.from_numpy(scene[k]).to(dev) for k in ("means", "quats", "scales", "opac", "feats", "K", "viewmat")}
    gauss = (t["means"], t["quats"], t["scales"], t["opac"])
    td = torch.from_numpy(prompts).to(dev)
    colors = torch.rand(scene["means"].shape[0], 3, generator=torch.Generator().manual_seed(2)).to(dev)
    mask2d, frame = next(gsbp_amd.render_prompt_mask(*gauss, t["feats"], t["viewmat"][None], t["K"], W, H, td, 1, colors=colors))
    # the literal form: D-channel render, F.normalize, matmul, compare
    with torch.no_grad():
        rendered = gsbp_amd.rasterization(*gauss, t["feats"], t["viewmat"][None], t["K"][None], W, H, want_meta=False)[0][0]
        rgb = gsbp_amd.rasterization(*gauss, colors, t["viewmat"][None], t["K"][None], W, H, want_meta=False)[0][0]
    score = F.normalize(rendered, dim=-1) @ td.T
    literal = score[..., :1].max(dim=2)[0] > score[..., 1:].max(dim=2)[0]
    dec = torch.from_numpy((margin > slack) & covered).reshape(H, W).to(dev)
    cov = torch.from_numpy(covered).reshape(H, W).to(dev)
    und = float((cov & ~dec).sum()) / float(cov.sum())
    print(f"covered {int(cov.sum())} pixels, undecided {100 * und:.3f} %, masks differ at {int((mask2d != literal).sum())} pixels")
    assert und <= 0.01
    assert mask2d.dtype == torch.bool and mask2d.shape == (H, W)
    assert torch.equal(mask2d[dec], literal[dec])
    assert 0.05 <= float(mask2d[cov].float().mean()) <= 0.95
    lit_frame = seg.overlay((rgb * 255.0).clamp(0.0, 255.0).to(torch.uint8), literal)
    same = mask2d == literal
    assert frame.dtype == torch.uint8 and frame.shape == (H, W, 3) and torch.equal(frame[same], lit_frame[same])
    assert next(gsbp_amd.render_prompt_mask(*gauss, t["feats"], t["viewmat"][None], t["K"], W, H, td, 1))[1] is None


# ---- 12. a click session ----------------------------------------------------------------------------------------------------------
def test_click_session_end_to_end(dev):
    scene = ref.two_blob_scene()
    W, H = scene["width"], scene["height"]
    t = {k: torch.from_numpy(scene[k]).to(dev) for k in ("means", "quats", "scales", "opac", "feats", "K", "viewmat")}
    gauss = (t["means"], t["quats"], t["scales"], t["opac"])
    first, second = scene["pixels"]
    vecs, depth, alpha = gsbp_amd.probe_pixels(*gauss, t["feats"], t["viewmat"], t["K"], W, H, [list(first), list(second)])
    assert float(alpha.min()) > 0.5 and 2.0 < float(depth[0] / alpha[0]) < 4.0
    session = gsbp_amd.ClickSession(t["feats"])
    assert session.mask() is None
    session.add_positive(vecs[0], position=first)
    session.add_negative(vecs[1], position=second)
    mask = session.mask()
    assert mask.dtype == torch.bool and mask.shape == (t["feats"].shape[0],) and 0.3 < float(mask.float().mean()) < 0.7
    splats = dict(means=t["means"], rotation=t["quats"], scaling=t["scales"].log(), opacity=torch.logit(t["opac"]))
    extracted, deleted = gsbp_amd.apply_mask3d(splats, mask)
    assert extracted["means"].shape[0] + deleted["means"].shape[0] == t["means"].shape[0]
    g = (extracted["means"], extracted["rotation"], extracted["scaling"].exp(), torch.sigmoid(extracted["opacity"]))
    with torch.no_grad():
        white = torch.ones(g[0].shape[0], 3, device=dev)
        a = gsbp_amd.rasterization(*g, white, t["viewmat"][None], t["K"][None], W, H, want_meta=False)[1][0, ..., 0]
    assert float(a[first[1], first[0]]) > 0.5 and float(a[second[1], second[0]]) < 0.5
    session.remove_negative(0)
    with pytest.raises(gsbp_amd.GwbpError):
        session.mask()
