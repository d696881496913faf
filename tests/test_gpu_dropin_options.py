"""The arguments of the drop-in `rasterization()` that the rest of the suite leaves at their defaults -- near_plane, far_plane,
radius_clip, eps2d, sh_degree below 3, the depth render modes, more than one camera per call -- through the HIP kernels and
the Python host, against the CPU oracle (whose option branches tests/test_dropin_options_cpu.py holds against float64).

Bars: bit-exact for everything the suite already pins bit for bit (projection, lists, alphas, meta); 1e-5 for rendered colours
(test_render_forward_parity), scaled by max |z| for a depth channel; 2e-6 SH kernel against oracle (test_sh_rgb_render_through_shim)
and the derived bound of dropin_ref.sh_reference against float64; 1e-4 relative per row for a harvested gradient."""
import numpy as np
import pytest
import torch

import dropin_ref as ref
from util import npy, rel_row_err, scene_np, to_dev

import gsbp_amd
from gsbp_amd import rasterization
from gsbp_amd import synthetic as syn
from gsbp_amd.rasterization import LazyMeta, get_engine

pytestmark = pytest.mark.gpu
TOL = 1e-4

_SCENES, _ORACLE = {}, {}


def scene(name, dev, **over):
    """(cfg, device tensors, host arrays) of a seeded scene: made once, never written to."""
    key = (name, tuple(sorted(over.items())))
    if key not in _SCENES:
        cfg, sc = scene_np(name, **over)
        if over.get("n_views"):
            sc["vms"] = syn.make_cameras(cfg, n_views=over["n_views"])
        _SCENES[key] = (cfg, to_dev(sc, dev), npy(sc))
    return _SCENES[key]


def oracle_front(orc, h, cfg, v, **kw):
    """(projection, lists) of the oracle for view v under the clip keywords of orc.project: computed once per combination."""
    key = (id(h["means"]), cfg.width, cfg.height, v, tuple(sorted(kw.items())))
    if key not in _ORACLE:
        p = orc.project(h["means"], h["quats"], h["scales"], h["vms"][v], h["K"], cfg.width, cfg.height, **kw)
        _ORACLE[key] = (p, orc.bin_sort(p, cfg.width, cfg.height))
    return _ORACLE[key]


def clip_cases(orc, h, cfg, v):
    """name -> (rasterization() keywords, orc.project keywords): the values of dropin_ref.clip_parameters for this view."""
    cp = ref.clip_parameters(oracle_front(orc, h, cfg, v)[0])
    out = {}
    for name, keys in (("near", ("near",)), ("far", ("far",)), ("radius_clip", ("radius_clip",)), ("all", ("near", "far", "radius_clip"))):
        o = {k: cp[k] for k in keys}
        out[name] = ({{"near": "near_plane", "far": "far_plane"}.get(k, k): val for k, val in o.items()}, o)
    for e in (0.05, 1.0):
        out[f"eps2d_{e}"] = (dict(eps2d=e), dict(eps2d=e))
    return cp, out


CASES = ["near", "far", "radius_clip", "all", "eps2d_0.05", "eps2d_1.0"]


def bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_sensitive(orc, h, cfg, v, case, o_kw, cp):
    """The option changes the visible set (checked on the ORACLE), and Gaussians sit on the equality cuts."""
    p0 = oracle_front(orc, h, cfg, v)[0]
    p = oracle_front(orc, h, cfg, v, **o_kw)[0]
    n0, n1 = int((p0["radii"] > 0).sum()), int((p["radii"] > 0).sum())
    if case.startswith("eps2d"):
        assert n1 > 0 and not np.array_equal(p["radii"], p0["radii"]) and not np.array_equal(p["conics"], p0["conics"])
        return
    assert 0 < n1 < n0, (case, n1, n0)
    vis0 = p0["radii"] > 0
    if "near" in o_kw:
        assert (p0["depths"][vis0] == np.float32(cp["near"])).any()
    if "far" in o_kw:
        assert (p0["depths"][vis0] == np.float32(cp["far"])).any()
    if "radius_clip" in o_kw:
        assert (p0["radii"] == cp["radius_clip"]).any() and (p0["radii"] == cp["radius_clip"] + 1).any()


def assert_front_equals_oracle(eng, view, d, ref_p, ref_b):
    proj = eng.project(view, d["means"], d["quats"], d["scales"], d["opac"], want_outputs=True)
    bins = eng.bin_sort(view, want_outputs=True)
    st = eng.stats()
    n = ref_b["n_isect"]
    assert st["overflow"] == 0 and st["n_isect"] == n and st["n_visible"] == int((ref_p["radii"] > 0).sum())
    assert np.array_equal(proj["radii"].cpu().numpy(), ref_p["radii"])
    for k in ("means2d", "depths", "conics"):
        assert np.array_equal(bits(proj[k]), bits(ref_p[k])), f"{k} differs bitwise"
    assert np.array_equal(bins["isect_ids"][:n].cpu().numpy(), ref_b["isect_ids"])
    assert np.array_equal(bins["flatten_ids"][:n].cpu().numpy(), ref_b["flatten_ids"])
    assert np.array_equal(bins["tile_offsets"].cpu().numpy(), ref_b["tile_offsets"])


# ---- a. clip options through Engine.view / project / bin_sort -----------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("name", ["T0", "T1"])
def test_clip_options_projection_and_lists_bit_exact(orc, dev, name, case):
    cfg, d, h = scene(name, dev)
    eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev)
    for v in range(cfg.n_views):
        cp, cases = clip_cases(orc, h, cfg, v)
        r_kw, o_kw = cases[case]
        assert_sensitive(orc, h, cfg, v, case, o_kw, cp)
        view = eng.view(d["vms"][v], d["K"], cfg.width, cfg.height, **r_kw)
        assert_front_equals_oracle(eng, view, d, *oracle_front(orc, h, cfg, v, **o_kw))


def test_exact_cuts_through_the_kernel(orc, dev):
    """Depths exactly ON near and far are kept, one ulp outside is culled (`z < near || z > far` culls)."""
    s = ref.exact_cut_scene()
    d = {k: torch.from_numpy(s[k]).to(dev) for k in ("means", "quats", "scales", "opac")}
    vm, K = torch.from_numpy(s["viewmat"]), torch.from_numpy(s["K"])
    eng = gsbp_amd.Engine(s["means"].shape[0], s["W"], s["H"], device=dev)
    z, roles = s["means"][:, 2], s["roles"]
    for kw, o_kw, want in ((dict(near_plane=s["near"]), dict(near=s["near"]), z >= np.float32(s["near"])),
                           (dict(far_plane=s["far"]), dict(far=s["far"]), z <= np.float32(s["far"])),
                           (dict(near_plane=s["near"], far_plane=s["far"]), dict(near=s["near"], far=s["far"]),
                            (z >= np.float32(s["near"])) & (z <= np.float32(s["far"])))):
        ref_p = orc.project(s["means"], s["quats"], s["scales"], s["viewmat"], s["K"], s["W"], s["H"], **o_kw)
        assert np.array_equal(ref_p["radii"] > 0, want) and 0 < int(want.sum()) < z.size  # the oracle, against the construction
        view = eng.view(vm, K, s["W"], s["H"], **kw)
        assert_front_equals_oracle(eng, view, d, ref_p, orc.bin_sort(ref_p, s["W"], s["H"]))
        radii = eng.project(view, d["means"], d["quats"], d["scales"], d["opac"], want_outputs=True)["radii"].cpu().numpy()
        assert np.array_equal(radii > 0, want)
    for k in ("on_near", "above_near", "on_far", "below_far"):
        assert (radii[roles[k]] > 0).all(), k
    for k in ("below_near", "above_far"):
        assert not (radii[roles[k]] > 0).any(), k


# ---- b. the same options through rasterization() ------------------------------------------------------------------------------------
def _rgb(n, dev):
    return torch.rand(n, 3, generator=torch.Generator().manual_seed(5)).to(dev)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("name", ["T0", "T1"])
def test_clip_options_render_against_the_oracle(orc, dev, name, case):
    cfg, d, h = scene(name, dev)
    v = 0
    cp, cases = clip_cases(orc, h, cfg, v)
    r_kw, o_kw = cases[case]
    assert_sensitive(orc, h, cfg, v, case, o_kw, cp)
    rgb = _rgb(cfg.n_gaussians, dev)
    with torch.no_grad():
        out, alpha, meta = rasterization(d["means"], d["quats"], d["scales"], d["opac"], rgb, d["vms"][v][None], d["K"][None],
                                         cfg.width, cfg.height, **r_kw)
        out0, alpha0, _ = rasterization(d["means"], d["quats"], d["scales"], d["opac"], rgb, d["vms"][v][None], d["K"][None],
                                        cfg.width, cfg.height, want_meta=False)
    ref_p, ref_b = oracle_front(orc, h, cfg, v, **o_kw)
    want, want_alpha = orc.render(ref_p, ref_b, h["opac"], rgb.cpu().numpy(), cfg.width, cfg.height)
    err = float(np.abs(out[0].cpu().numpy() - want).max())
    print(f"{name} {case}: max |render - oracle| = {err:.2e}")
    assert err <= 1e-5
    assert np.array_equal(bits(alpha[0, ..., 0]), bits(want_alpha))
    assert not torch.equal(alpha, alpha0)  # the option reached the image
    assert np.array_equal(meta["gaussian_ids"].cpu().numpy(), np.nonzero(ref_p["radii"] > 0)[0])


@pytest.mark.parametrize("which", ["near", "far"])
@pytest.mark.parametrize("name", ["T0", "T1"])
def test_harvest_backward_under_a_clip_plane(orc, dev, name, which):
    """The reference's harvest (zeros [N, 512], (render * feats).sum().backward()) with a clip plane in the call."""
    cfg, d, h = scene(name, dev)
    v, D = 1, 512
    cp, cases = clip_cases(orc, h, cfg, v)
    r_kw, o_kw = cases[which]
    assert_sensitive(orc, h, cfg, v, which, o_kw, cp)
    feats = syn.make_feature_map(cfg, v, dim=D)
    table = torch.zeros(cfg.n_gaussians, D, device=dev, requires_grad=True)
    out, _, _ = rasterization(d["means"], d["quats"], d["scales"], d["opac"], table, d["vms"][v][None], d["K"][None],
                              cfg.width, cfg.height, want_meta=False, **r_kw)
    (out[0] * feats.to(dev)).sum().backward()
    Fr, dr = np.zeros((cfg.n_gaussians, D), np.float64), np.zeros(cfg.n_gaussians, np.float64)
    info = orc.backproject_view(h["means"], h["quats"], h["scales"], h["opac"], h["vms"][v], h["K"], cfg.width, cfg.height,
                                feats.numpy(), Fr, dr, **o_kw)
    assert info["n_pairs"] > 0
    err = rel_row_err(table.grad.cpu().numpy(), Fr)
    print(f"{name} {which}: harvest row error {err:.2e}")
    assert err <= TOL
    culled = oracle_front(orc, h, cfg, v, **o_kw)[0]["radii"] == 0
    assert not table.grad[torch.from_numpy(culled).to(dev)].any()


# ---- c. the front cache ---------------------------------------------------------------------------------------------------------------
def test_front_cache_keys_on_every_clip_option(orc, dev):
    cfg, d, h = scene("T1", dev)
    v = 0
    cp, _ = clip_cases(orc, h, cfg, v)
    rgb = _rgb(cfg.n_gaussians, dev)
    args = (d["means"], d["quats"], d["scales"], d["opac"], rgb, d["vms"][v][None], d["K"][None], cfg.width, cfg.height)
    eng = get_engine(dev, cfg.n_gaussians, cfg.width, cfg.height)

    def call(**kw):
        with torch.no_grad():
            out, alpha, _ = rasterization(*args, want_meta=False, **kw)
        return out[0].clone(), alpha[0, ..., 0].clone()

    def fresh(**kw):
        e = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev)
        view = e.view(d["vms"][v], d["K"], cfg.width, cfg.height, **kw)
        e.project(view, d["means"], d["quats"], d["scales"], d["opac"])
        e.bin_sort(view)
        assert not e.stats()["overflow"]
        return e.render_pixels(view, rgb)

    kw = {}
    base = call()
    gen = eng.generation
    assert all(torch.equal(a, b) for a, b in zip(call(), base)) and eng.generation == gen  # the identical call: served from the cache
    for key, val in (("near_plane", cp["near"]), ("far_plane", cp["far"]), ("radius_clip", cp["radius_clip"]), ("eps2d", 0.05)):
        kw[key] = val
        before = call(**{k: x for k, x in kw.items() if k != key})  # the cache holds the view WITHOUT this option
        gen = eng.generation
        got = call(**kw)
        assert eng.generation == gen + 1, f"a changed {key} was served from the cache"
        want = fresh(**kw)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), key
        assert not torch.equal(got[1], before[1]), key
        again = call(**kw)
        assert eng.generation == gen + 1 and torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])


# ---- d. the other consumers of raster_kw ----------------------------------------------------------------------------------------------
def test_label_maps_probe_and_field_agreement_forward_the_clip_options(orc, dev):
    cfg, d, h = scene("T1", dev)
    v = 0
    cp, cases = clip_cases(orc, h, cfg, v)
    for case in ("near", "radius_clip"):
        assert_sensitive(orc, h, cfg, v, case, cases[case][1], cp)
    gauss = (d["means"], d["quats"], d["scales"], d["opac"])
    N, W, H = cfg.n_gaussians, cfg.width, cfg.height
    vm, K = d["vms"][v], d["K"]
    g = torch.Generator().manual_seed(8)
    near = dict(near_plane=cp["near"])
    # render_label_maps == rasterization() of the one-hot table
    k = 7
    labels = torch.randint(0, k, (N,), generator=g, dtype=torch.int32)
    onehot = torch.nn.functional.one_hot(labels.long(), k).float().to(dev)
    with torch.no_grad():
        want, want_alpha, _ = rasterization(*gauss, onehot, vm[None], K[None], W, H, want_meta=False, **near)
        _, alpha0, _ = rasterization(*gauss, onehot, vm[None], K[None], W, H, want_meta=False)
    maps, alphas = gsbp_amd.render_label_maps(*gauss, labels.to(dev), k, vm, K, W, H, **near)
    assert torch.equal(maps, want[0]) and torch.equal(alphas, want_alpha[0, ..., 0])
    assert not torch.equal(alphas, alpha0[0, ..., 0])
    # probe_pixels == rasterization(render_mode="RGB+D") at the pixels
    feats = torch.randn(N, 16, generator=g).to(dev)
    with torch.no_grad():
        full, full_alpha, _ = rasterization(*gauss, feats, vm[None], K[None], W, H, render_mode="RGB+D", want_meta=False, **near)
    xy = torch.stack([torch.randint(0, W, (64,), generator=g), torch.randint(0, H, (64,), generator=g)], 1).to(dev)
    got, depth, a = gsbp_amd.probe_pixels(*gauss, feats, vm, K, W, H, xy, **near)
    at = full[0][xy[:, 1], xy[:, 0]]
    assert torch.equal(got, at[:, :16]) and torch.equal(depth, at[:, 16]) and torch.equal(a, full_alpha[0, ..., 0][xy[:, 1], xy[:, 0]])
    assert int((a > 0).sum()) >= 8 and not torch.equal(a, alpha0[0, ..., 0][xy[:, 1], xy[:, 0]])
    # render_field_agreement: rasterization()'s alpha, and the sums of ITS render
    rc = dict(radius_clip=cp["radius_clip"])
    D = 32
    field = torch.randn(N, D, generator=g).to(dev)
    fmap = torch.randn(H, W, D, generator=g).to(dev)
    with torch.no_grad():
        r, r_alpha, _ = rasterization(*gauss, field, vm[None], K[None], W, H, want_meta=False, **rc)
    out = gsbp_amd.render_field_agreement(*gauss, field, fmap, vm, K, W, H, **rc)
    assert torch.equal(out["alpha"], r_alpha[0, ..., 0]) and not torch.equal(out["alpha"], alpha0[0, ..., 0])
    r64, m64 = r[0].double(), fmap.double()
    for name, terms in (("dot", r64 * m64), ("rr", r64 * r64), ("l2", (r64 - m64) ** 2)):
        err = (out[name].double() - terms.sum(-1)).abs()
        bound = (D + 2) * ref.U * terms.abs().sum(-1)  # (the bar of test_sums_equal_float64_sums_of_the_librarys_render)
        assert bool((err <= bound).all()), name


# ---- e. spherical harmonics -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree,K,N", ref.SH_GRID)
def test_sh_colors_against_oracle_and_float64(orc, dev, degree, K, N):
    eng = gsbp_amd.Engine(N, 16, 16, device=dev)
    for case in ref.sh_cases(degree, K, N):
        got = eng.sh_colors(degree, torch.from_numpy(case["means"]).to(dev), torch.from_numpy(case["coeffs"]).to(dev),
                            case["campos"].tolist()).cpu().numpy()
        o = orc.sh_colors(degree, case["means"], case["coeffs"], case["campos"])
        want, bound = ref.sh_reference(degree, case["means"], case["coeffs"], case["campos"])
        err = np.abs(got.astype(np.float64) - want)
        print(f"degree {degree} K {K} N {N}: max |kernel - oracle| = {float(np.abs(got - o).max()):.2e}, "
              f"max err / bound against float64 = {float((err / bound).max()):.3f}")
        assert got.shape == (N, 3) and np.isfinite(got).all()
        assert np.abs(got - o).max() < 2e-6
        assert (err <= bound).all()
        if case["clamped"] is not None:
            assert (want[case["clamped"]] == 0.0).all() and np.array_equal(got[case["clamped"]], np.zeros(3, np.float32))
        if case["at_camera"] is not None:
            i = case["at_camera"]
            dc = np.maximum(0.28209479177387814 * case["coeffs"][i, 0].astype(np.float64) + 0.5, 0.0)
            assert (np.abs(got[i] - dc) <= bound[i]).all()


def test_sh_degree_below_the_stored_bands_through_rasterization(dev):
    cfg, d, _ = scene("T1", dev)
    N, W, H = cfg.n_gaussians, cfg.width, cfg.height
    sh = syn.make_sh_coeffs(cfg, 3).to(dev)
    sh[:, 1:] *= 4.0  # (bands that show in the image)
    gauss = (d["means"], d["quats"], d["scales"], d["opac"])
    vms, K = d["vms"][:1], d["K"][None]
    eng = gsbp_amd.Engine(N, W, H, device=dev)
    campos = eng.campos(eng.view(d["vms"][0], d["K"], W, H))
    imgs = {}
    with torch.no_grad():
        for degree in (0, 1, 2, 3):
            out, alpha, _ = rasterization(*gauss, sh, vms, K, W, H, sh_degree=degree, want_meta=False)
            imgs[degree] = out[0].clone()
            cols = eng.sh_colors(degree, d["means"], sh, campos)
            want, want_alpha, _ = rasterization(*gauss, cols, vms, K, W, H, want_meta=False)
            assert torch.equal(imgs[degree], want[0]) and torch.equal(alpha, want_alpha)
            nb = (degree + 1) ** 2
            tight, _, _ = rasterization(*gauss, sh[:, :nb].contiguous(), vms, K, W, H, sh_degree=degree, want_meta=False)
            assert torch.equal(tight[0], want[0])  # K = (degree + 1)^2 exactly
    for degree in (0, 1, 2):
        assert not torch.equal(imgs[degree], imgs[degree + 1])  # the degree is not ignored


# ---- f. depth render modes ------------------------------------------------------------------------------------------------------------
def _sparse_t1(dev):
    """T1's last 1500 Gaussians at 0.6 of their size: some pixels stay uncovered (alpha == 0)."""
    cfg, d, h = scene("T1", dev)
    key = ("T1sparse",)
    if key not in _SCENES:
        hs = {k: (np.ascontiguousarray(h[k][-1500:]) if k in ("means", "quats", "scales", "opac") else h[k]) for k in h}
        hs["scales"] = (hs["scales"] * np.float32(0.6)).astype(np.float32)
        _SCENES[key] = (cfg, {k: torch.from_numpy(x).to(dev) for k, x in hs.items()}, hs)
    return _SCENES[key]


@pytest.mark.parametrize("name", ["T0", "T1sparse"])
def test_depth_render_modes(orc, dev, name):
    cfg, d, h = _sparse_t1(dev) if name == "T1sparse" else scene(name, dev)
    N, W, H = h["means"].shape[0], cfg.width, cfg.height
    v = 0
    gauss = (d["means"], d["quats"], d["scales"], d["opac"])
    vms, K = d["vms"][v][None], d["K"][None]
    rgb = _rgb(N, dev)
    outs = {}
    with torch.no_grad():
        for mode in ("RGB", "D", "ED", "RGB+D", "RGB+ED"):
            o, a, _ = rasterization(*gauss, rgb, vms, K, W, H, render_mode=mode, want_meta=False)
            outs[mode] = (o[0].clone(), a[0].clone())
    alpha = outs["RGB"][1]
    assert all(torch.equal(outs[m][1], alpha) for m in outs)
    assert [outs[m][0].shape[-1] for m in ("RGB", "D", "ED", "RGB+D", "RGB+ED")] == [3, 1, 1, 4, 4]
    # "D" against the oracle's render of the camera-z column
    vm = h["vms"][v]
    z = (h["means"] @ vm[:3, :3].T + vm[:3, 3])[:, 2:3].astype(np.float32)
    ref_p, ref_b = oracle_front(orc, h, cfg, v)
    want, want_alpha = orc.render(ref_p, ref_b, h["opac"], z, W, H)
    bar = 1e-5 * float(np.abs(z).max())
    err = float(np.abs(outs["D"][0].cpu().numpy() - want).max())
    print(f"{name}: max |D - oracle| = {err:.2e} (bar {bar:.2e})")
    assert err <= bar and float(want.max()) > 1.0
    assert np.array_equal(bits(alpha[..., 0]), bits(want_alpha))
    assert float(np.abs(outs["RGB+D"][0][..., 3:].cpu().numpy() - want).max()) <= bar
    # expected depth = accumulated depth / alpha, finite where nothing was rendered
    if name == "T1sparse":
        assert int((alpha == 0).sum()) > 0, "the scene leaves no pixel uncovered"
    assert torch.equal(outs["ED"][0], outs["D"][0] / alpha.clamp_min(1e-10))
    assert torch.equal(outs["RGB+ED"][0][..., 3:], outs["RGB+D"][0][..., 3:] / alpha.clamp_min(1e-10))
    assert torch.equal(outs["RGB+ED"][0][..., :3], outs["RGB"][0]) and torch.equal(outs["RGB+D"][0][..., :3], outs["RGB"][0])
    for m in ("ED", "RGB+ED"):
        assert bool(torch.isfinite(outs[m][0]).all())
        assert not bool(outs[m][0][..., -1][alpha[..., 0] == 0].any())
    covered = alpha[..., 0] > 0.5
    ed = outs["ED"][0][..., 0][covered]
    assert float(ed.min()) >= float(z.min()) * (1 - 1e-5) and float(ed.max()) <= float(z.max()) * (1 + 1e-5)  # a weighted mean of depths
    # backgrounds whose depth entry is zero: colours get (1 - alpha) bg, the depth channel is untouched -- in either order of
    # "divide" and "add the background"
    with torch.no_grad():
        for mode in outs:
            nc = outs[mode][0].shape[-1]
            bg = torch.tensor([[0.2, 0.4, 0.6, 0.0]], device=dev)[:, :nc] if "RGB" in mode else torch.zeros(1, 1, device=dev)
            o, a, _ = rasterization(*gauss, rgb, vms, K, W, H, render_mode=mode, backgrounds=bg, want_meta=False)
            o = o[0]
            assert torch.equal(a[0], alpha)
            if "RGB" in mode:
                assert torch.equal(o[..., :3], outs[mode][0][..., :3] + (1.0 - alpha) * bg[0, :3]), mode
            if "D" in mode:
                assert torch.equal(o[..., -1], outs[mode][0][..., -1]), mode


# ---- g. more than one camera per call -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [None, (64, 64)], ids=["96x64", "64x64_16_tiles"])
@pytest.mark.parametrize("C", [2, 3])
def test_cameras_in_one_call_equal_one_camera_calls(orc, dev, C, size):
    over = dict(n_views=3, **(dict(width=size[0], height=size[1]) if size else {}))
    cfg, d, h = scene("T0", dev, **over)
    N, W, H = cfg.n_gaussians, cfg.width, cfg.height
    gauss = (d["means"], d["quats"], d["scales"], d["opac"])
    vms, Ks = d["vms"][:C], d["K"][None].expand(C, 3, 3)
    g = torch.Generator().manual_seed(21)
    shared = torch.rand(N, 3, generator=g).to(dev)
    per_cam = torch.rand(C, N, 3, generator=g).to(dev)
    per_cam_sh = (0.3 * torch.randn(C, N, 16, 3, generator=g)).to(dev)
    bgs = torch.rand(C, 3, generator=g).to(dev)
    assert not torch.equal(d["vms"][0], d["vms"][1]) and not torch.equal(d["vms"][1], d["vms"][2])

    def single(c, colors, **kw):
        if kw.get("backgrounds") is not None:
            kw["backgrounds"] = kw["backgrounds"][c:c + 1]
        with torch.no_grad():
            o, a, m = rasterization(*gauss, colors, vms[c:c + 1], Ks[c:c + 1], W, H, **kw)
        return o[0].clone(), a[0].clone(), m

    for colors, pick, kw in ((shared, lambda c: shared, {}), (per_cam, lambda c: per_cam[c], {}),
                             (per_cam_sh, lambda c: per_cam_sh[c], dict(sh_degree=3)),
                             (per_cam, lambda c: per_cam[c], dict(backgrounds=bgs)),
                             (shared, lambda c: shared, dict(render_mode="RGB+ED"))):
        with torch.no_grad():
            out, alphas, _ = rasterization(*gauss, colors, vms, Ks, W, H, want_meta=False, **kw)
        assert out.shape[:3] == (C, H, W) and alphas.shape == (C, H, W, 1)
        for c in range(C):
            o, a, _ = single(c, pick(c), want_meta=False, **kw)
            assert torch.equal(out[c], o) and torch.equal(alphas[c], a), (c, sorted(kw))
        assert not torch.equal(alphas[0], alphas[1])

    # the cameras' renders against the oracle, and every key of the packed meta
    with torch.no_grad():
        out, alphas, meta = rasterization(*gauss, per_cam, vms, Ks, W, H)
    per_camera = []
    for c in range(C):
        p, b = oracle_front(orc, h, cfg, c)
        per_camera.append(dict(proj=p, bins=b))
        want, want_alpha = orc.render(p, b, h["opac"], per_cam[c].cpu().numpy(), W, H)
        assert np.abs(out[c].cpu().numpy() - want).max() <= 1e-5
        assert np.array_equal(bits(alphas[c, ..., 0]), bits(want_alpha))
    want = ref.packed_meta(per_camera, opacities=h["opac"], width=W, height=H)
    assert len(want["isect_ids"]) > 0 and len(np.unique(want["camera_ids"])) == C
    keys = set(LazyMeta._LAZY) | set(dict.keys(meta))
    assert keys == set(want), keys ^ set(want)
    for k in sorted(keys):
        got = meta[k]
        if torch.is_tensor(got):
            assert tuple(got.shape) == want[k].shape, (k, tuple(got.shape), want[k].shape)
            assert np.array_equal(bits(got), bits(want[k])), k
        else:
            assert got == want[k], k
    assert tuple(meta["isect_offsets"].shape) == (C, -(-H // 16), -(-W // 16))
    if size:  # 16 tiles: floor(log2(16)) + 1 = 5 tile bits, so camera 1 starts at bit 37
        last = int(meta["isect_ids"][-1])
        assert last >> 37 == C - 1 and (last >> 32) & 31 < 16
    # want_meta=False: the eager dict only
    with torch.no_grad():
        _, _, eager = rasterization(*gauss, per_cam, vms, Ks, W, H, want_meta=False)
    assert type(eager) is dict and set(eager) == {"tile_width", "tile_height", "width", "height", "tile_size", "n_cameras"}
    assert eager["n_cameras"] == C and "isect_ids" not in eager

    # antialiased: compensations and compensated opacities, camera by camera
    with torch.no_grad():
        _, _, meta_aa = rasterization(*gauss, shared, vms, Ks, W, H, rasterize_mode="antialiased")
    comp = meta_aa["compensations"]
    start = 0
    for c in range(C):
        _, _, m1 = single(c, shared, rasterize_mode="antialiased")
        n = m1["gaussian_ids"].numel()
        assert n > 0 and torch.equal(meta_aa["gaussian_ids"][start:start + n], m1["gaussian_ids"])
        assert torch.equal(comp[start:start + n], m1["compensations"])
        assert torch.equal(meta_aa["opacities"][start:start + n], m1["opacities"])
        assert torch.equal(m1["opacities"], d["opac"][m1["gaussian_ids"]] * m1["compensations"])
        assert bool((m1["compensations"] > 0).all()) and bool((m1["compensations"] < 1).any())
        start += n
    assert start == comp.numel() == meta_aa["camera_ids"].numel()
