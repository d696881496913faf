"""The front stage (gwbp_project -> gwbp_bin_sort -> a blend) ON the sizes at which it changes its code path, against the CPU oracle.

    A  tile counts 1 / 256 / 272 / 65 536 / 80 000: the 1, 2 and 3 byte-passes of the tile sort, and one consumer for every place
       that re-derives the buffer the sorted lists end in (fin = sort_passes & 1: the storing, fused and token blends of blend.hip,
       token_kernel.h, query_kernel.h, render.hip, label_render.hip)
    B  depth ties (at most three depth values, culled Gaussians interleaved by index) through k_sort_small<4>, <8>, <12> and the
       multi-block radix passes, at N = 4096/4097, 8192/8193, 12 288/12 289 and beyond; lists longer than k_tile_order's last bucket
    C  n_isect on the boundary of a 4096-key sort block, with isect_cap == n_isect and with ample capacity
    D  isect_cap == n (exact) and n - 1 (bit 0, an EMPTY view for every blend / consumer family), for both counters
       (k_sort_small's tail: N <= 12 288; k_scan_blocksums: above)
    E  pair_cap == pool_used (fits) and pool_used - 1 (bit 1 and no other)
    F  after every overflow of D and E the same workspace projects a fitting view, which must equal that view on a fresh workspace

Where the seven fin sites are reached (each test runs at 1, 2 and 3 passes unless stated):
    blend.hip launch_blend            test_weight_store_and_scatter_*, test_fused_blend_scatter_* (both forms), test_fused_encoded_blend_*
    blend.hip launch_blend_render     test_rgb_blend_* (with the half-tile lists of the 256-channel scatter)
    blend.hip launch_blend_tokens     test_token_blend_and_apply_* -- 1 and 2 passes only: the token path takes at most 256 x 256 tiles
    token_kernel.h                    the same test, the same limit
    query_kernel.h                    test_probe_pixels_*
    render.hip                        test_render_pixels_*
    label_render.hip                  test_render_labels_*
gwbp_scatter derives no fin (it reads the headers the blend left); D = 3 takes k_scatter_full's small form, D = 65 the generic k_scatter.

Scenes and their conditions: tests/front_boundary_scenes.py (asserted on the oracle alone in tests/test_front_boundaries_cpu.py and
again here).  Bars: indices, per-pair weights and alphas of gwbp_blend_weights bit for bit; F and d within 1e-4 per row of the oracle
and within 1e-5 between two HIP runs; renders, labels and probes as in their own tests."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import front_boundary_scenes as fb
import label_render_ref
import test_gpu_workspace_sequences as ws
from util import rel_row_err, sort_pairs

import gsbp_amd

pytestmark = pytest.mark.gpu
TOL = 1e-4      # F and d against the oracle (test_gpu_parity.TOL)
GAUSS = ("means", "quats", "scales", "opac")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _on_dev(sc, dev):
    return [torch.from_numpy(sc[k]).to(dev) for k in GAUSS]


def _view_of(eng, sc):
    return eng.view(torch.from_numpy(sc["viewmat"]), torch.from_numpy(sc["K"]), sc["W"], sc["H"])


def _front(eng, sc, g):
    """project + bin_sort with the sorted lists exported; asserts them exact against the oracle."""
    view = _view_of(eng, sc)
    eng.project(view, *g)
    bins = eng.bin_sort(view, want_outputs=True)
    st = eng.stats()
    proj, ref = fb.front(sc)
    n = ref["n_isect"]
    assert st["overflow"] == 0 and st["n_isect"] == n, (st, n)
    assert st["n_visible"] == int((proj["radii"] > 0).sum())
    assert np.array_equal(bins["tile_offsets"].cpu().numpy(), ref["tile_offsets"]), "tile_offsets differ"
    assert np.array_equal(bins["flatten_ids"][:n].cpu().numpy(), ref["flatten_ids"]), "flatten_ids differ: (tile, depth, index) order"
    assert np.array_equal(bins["isect_ids"][:n].cpu().numpy(), ref["isect_ids"]), "isect_ids differ"
    return view


def _store_exact(eng, view, sc, blend=None):
    """gwbp_blend_weights (or another storing blend that returns its alpha map): the (Gaussian, pixel) pairs, their weights and
    the alpha map bit for bit."""
    alphas = eng.blend_weights(view, want_alphas=True) if blend is None else blend()
    gid, pix, w = eng.dump_pairs(view)
    st = eng.stats()
    rk, rw, ralpha = fb.pairs(sc)
    assert st["overflow"] == 0 and st["n_pairs"] == len(rk) > 0, (st, len(rk))
    k, w = sort_pairs(gid.cpu().numpy(), pix.cpu().numpy(), w.cpu().numpy())
    assert np.array_equal(k, rk), "set of contributing (gaussian, pixel) pairs differs"
    assert np.array_equal(_bits(w), _bits(rw)), "weights differ bitwise"
    assert np.array_equal(_bits(alphas.cpu().numpy()), _bits(ralpha)), "alphas differ bitwise"


def _oracle_field(orc, sc, fmap):
    """F, d (float64) of the oracle's back-projection of fmap [H, W, D] (numpy float32) on the scene's cached front."""
    proj, bins = fb.front(sc)
    n = sc["means"].shape[0]
    F, d = np.zeros((n, fmap.shape[2]), np.float64), np.zeros(n, np.float64)
    n_pairs, _ = orc.blend_scatter(proj, bins, sc["opac"], np.ascontiguousarray(fmap), F, d, sc["W"], sc["H"])
    assert n_pairs == len(fb.pairs(sc)[0]) and d.max() > 0
    return F, d


def _assert_field(F, d, Fr, dr, what):
    eF, ed = rel_row_err(F.cpu().numpy(), Fr), rel_row_err(d.cpu().numpy()[:, None], dr[:, None])
    print(f"{what}: rel_row_err F {eF:.2e} d {ed:.2e}")
    assert eF <= TOL and ed <= TOL, what


def _map(sc, D, dev, seed=0, positive=False):
    """A feature map [H, W, D] made on the device (the widest image has 10.9 M pixels), and its host copy."""
    g = torch.Generator(device=dev).manual_seed(900 + seed)
    f = torch.randn(sc["H"], sc["W"], D, device=dev, generator=g)
    if positive:  # a row of one to three signed channels can cancel to nearly nothing (test_gpu_parity does the same for D < 4)
        f = f.abs()
    return f, f.cpu().numpy()


# ---- A. the pass count of the tile sort ----------------------------------------------------------------------------------------------------
_TILE_CASES = {}


def tile_case(dev, name):
    """One engine per tile-count scene with the view projected and sorted (asserted exact): every consumer test blends from it."""
    if name not in _TILE_CASES:
        fb.check_tile_scene(name)
        sc = fb.tile_scene(name)
        n = sc["means"].shape[0]
        # (the default pair_cap is 128 x W x H entries; a tile that stores anything takes a 1024-entry page of its shard)
        caps = dict(isect_cap=1 << 15, pair_cap=1 << 24) if sc["H"] == 17 else {}
        eng = gsbp_amd.Engine(n, sc["W"], sc["H"], device=dev, **caps)
        g = _on_dev(sc, dev)
        _TILE_CASES[name] = dict(sc=sc, eng=eng, g=g, view=_front(eng, sc, g), n=n)
    c = _TILE_CASES[name]
    c["eng"].set_narrow_scatter(True)
    c["eng"].set_split_encoder(False)
    return c


TILE_NAMES = list(fb.TILE_SCENES)
TOKEN_MAPS = {"t1": (1, 1), "t256": (5, 7), "t272": (7, 9)}  # the images inside gwbp_scatter_tokens' 4096 x 4096 limit


@pytest.mark.parametrize("name", TILE_NAMES)
def test_tile_sort_is_exact_at_every_pass_count(orc, dev, name):
    c = tile_case(dev, name)  # (_front asserts isect_ids, flatten_ids, tile_offsets, n_isect, n_visible)
    assert fb.sort_passes(fb.n_tiles(c["sc"]["W"], c["sc"]["H"])) == fb.TILE_PASSES[name]


@pytest.mark.parametrize("name", TILE_NAMES)
def test_weight_store_and_scatter_at_every_pass_count(orc, dev, name):
    """blend.hip's storing blend reads the sorted lists; gwbp_scatter then reads the store it left."""
    c = tile_case(dev, name)
    sc, eng, view = c["sc"], c["eng"], c["view"]
    _store_exact(eng, view, sc)
    for D in (3,) if sc["H"] == 17 else (3, 65):  # D <= 64: k_scatter_full's small form; 65: the generic k_scatter
        fmap, fnp = _map(sc, D, dev, positive=True)
        F, d = torch.zeros(c["n"], D, device=dev), torch.zeros(c["n"], device=dev)
        eng.scatter(view, fmap, F, d)
        assert eng.stats()["overflow"] == 0
        _assert_field(F, d, *_oracle_field(orc, sc, fnp), f"{name} scatter D={D}")


@pytest.mark.parametrize("name", TILE_NAMES)
def test_fused_blend_scatter_at_every_pass_count(orc, dev, name):
    """gwbp_blend_scatter at D = 3: a wave per quarter tile up to 4096 tiles, a wave per tile above."""
    c = tile_case(dev, name)
    sc, eng, view = c["sc"], c["eng"], c["view"]
    fmap, fnp = _map(sc, 3, dev, seed=1, positive=True)
    F, d = torch.zeros(c["n"], 3, device=dev), torch.zeros(c["n"], device=dev)
    alphas = eng.blend_scatter(view, fmap, F, d, want_alphas=True)
    st = eng.stats()
    assert st["overflow"] == 0 and st["n_pairs"] == len(fb.pairs(sc)[0])
    assert np.array_equal(_bits(alphas.cpu().numpy()), _bits(fb.pairs(sc)[2]))
    _assert_field(F, d, *_oracle_field(orc, sc, fnp), f"{name} blend_scatter")


def _colors(n, D, dev, seed=3):
    t = torch.rand(n, D, generator=torch.Generator().manual_seed(seed))
    return t.to(dev), t.numpy()


@pytest.mark.parametrize("name", TILE_NAMES)
def test_rgb_blend_at_every_pass_count(orc, dev, name):
    """blend.hip's launcher of the storing blend WITH the RGB composite (gwbp_blend_weights_rgb), here with the half-tile lists of the
    256-channel scatter: the same store bit for bit, and the image of gwbp_render_pixels bit for bit (include/gwbp.h)."""
    c = tile_case(dev, name)
    sc, eng, view = c["sc"], c["eng"], c["view"]
    colors, _ = _colors(c["n"], 3, dev)
    out = {}

    def blend():
        out["image"], alphas = eng.blend_weights_rgb(view, colors, want_alphas=True)
        return alphas

    eng.set_narrow_scatter(False)
    _store_exact(eng, view, sc, blend)
    assert eng.stats()["blend_kind"] == 1
    eng.set_narrow_scatter(True)
    assert torch.equal(out["image"], eng.render_pixels(view, colors)[0])


@pytest.mark.parametrize("name", TILE_NAMES)
def test_render_pixels_at_every_pass_count(orc, dev, name):
    """render.hip, against the oracle's render (1e-5, as test_render_forward_parity; alphas 1e-6, as the sequences file)."""
    c = tile_case(dev, name)
    sc, eng, view = c["sc"], c["eng"], c["view"]
    colors, cnp = _colors(c["n"], 3, dev)
    image, alphas = eng.render_pixels(view, colors)
    proj, bins = fb.front(sc)
    ref, ralpha = orc.render(proj, bins, sc["opac"], cnp, sc["W"], sc["H"])
    assert ref.max() > 0.05
    err, err_a = float(np.abs(image.cpu().numpy() - ref).max()), float(np.abs(alphas.cpu().numpy() - ralpha).max())
    print(f"{name} render_pixels: max |image - oracle| {err:.2e}, alphas {err_a:.2e}")
    assert err <= 1e-5 and err_a <= 1e-6


@pytest.mark.parametrize("name", TILE_NAMES)
def test_render_labels_at_every_pass_count(orc, dev, name):
    """label_render.hip: bit for bit the pixel render of the one-hot table, within 1e-4 of the oracle's (test_gpu_label_render)."""
    c = tile_case(dev, name)
    sc, eng, view = c["sc"], c["eng"], c["view"]
    K = 3
    lab = (np.arange(c["n"]) % 5 - 1).astype(np.int32)  # -1 and 3 belong to no class
    table = label_render_ref.one_hot(lab, K)
    maps, alphas, _, _ = eng.render_labels(view, torch.from_numpy(lab).to(dev), K)
    want, want_alpha = eng.render_pixels(view, torch.from_numpy(table).to(dev))
    assert torch.equal(maps, want) and torch.equal(alphas, want_alpha)
    proj, bins = fb.front(sc)
    o_maps, o_alphas = orc.render(proj, bins, sc["opac"], table, sc["W"], sc["H"])
    err, err_a = float(np.abs(maps.cpu().numpy() - o_maps).max()), float(np.abs(alphas.cpu().numpy() - o_alphas).max())
    print(f"{name} render_labels: max |maps - oracle| {err:.2e}, alphas {err_a:.2e}")
    assert err <= 1e-4 and err_a <= 1e-4 and o_maps.max() > 0.2


@pytest.mark.parametrize("name", TILE_NAMES)
def test_probe_pixels_at_every_pass_count(orc, dev, name):
    """query_kernel.h: the probe equals the full pixel render at its pixels bit for bit (test_gpu_segment), which the test above
    holds against the oracle; the depth column against the oracle's render of the projected depths."""
    c = tile_case(dev, name)
    sc, eng, view = c["sc"], c["eng"], c["view"]
    W, H = sc["W"], sc["H"]
    proj, bins = fb.front(sc)
    vis = np.nonzero(proj["radii"] > 0)[0]
    pick = vis[:: max(1, len(vis) // 200)]  # pixels under the centres of visible Gaussians, all over the tile ids
    xy = np.floor(proj["means2d"][pick]).astype(np.int64)
    xy = np.concatenate([np.clip(xy, 0, [W - 1, H - 1]), [[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1]]]).astype(np.int32)
    table, tnp = _colors(c["n"], 5, dev, seed=4)
    out, depth, alpha = eng.probe_pixels(view, torch.from_numpy(xy).to(dev), table)
    image, alphas = eng.render_pixels(view, table)
    ix = torch.from_numpy(xy.astype(np.int64)).to(dev)
    assert torch.equal(out, image[ix[:, 1], ix[:, 0]]) and torch.equal(alpha, alphas[ix[:, 1], ix[:, 0]])
    assert int((alpha > 0).sum()) >= min(len(pick), 100) // 2, "the probed pixels hit nothing"
    ref, _ = orc.render(proj, bins, sc["opac"], np.ascontiguousarray(proj["depths"][:, None]), W, H)
    err = float(np.abs(depth.cpu().numpy() - ref[xy[:, 1], xy[:, 0], 0]).max())
    print(f"{name} probe depth: max |depth - oracle| {err:.2e}")
    assert err <= 1e-5 * float(proj["depths"].max())


@pytest.mark.parametrize("name", list(TOKEN_MAPS))
def test_token_blend_and_apply_at_every_pass_count_it_takes(orc, dev, name):
    """blend.hip's token blend and token_kernel.h, against the oracle fed the nearest-upsampled map."""
    c = tile_case(dev, name)
    sc, eng, view = c["sc"], c["eng"], c["view"]
    lh, lw = TOKEN_MAPS[name]
    D = 64
    assert gsbp_amd.Engine.token_geometry_ok(lh, lw, sc["H"], sc["W"])
    low = torch.randn(lh, lw, D, generator=torch.Generator().manual_seed(6))
    up = TF.interpolate(low.permute(2, 0, 1)[None], size=(sc["H"], sc["W"]), mode="nearest")[0].permute(1, 2, 0)
    alphas = eng.blend_tokens(view, lh, lw, want_alphas=True)
    F, d = torch.zeros(c["n"], D, device=dev), torch.zeros(c["n"], device=dev)
    eng.scatter_tokens(view, low.to(dev), F, d)
    st = eng.stats()
    assert st["overflow"] == 0 and st["n_pairs"] == len(fb.pairs(sc)[0]) and st["blend_kind"] == 3
    assert np.array_equal(_bits(alphas.cpu().numpy()), _bits(fb.pairs(sc)[2]))
    _assert_field(F, d, *_oracle_field(orc, sc, up.numpy()), f"{name} tokens")


@pytest.mark.parametrize("split", [False, True], ids=["one_wave_per_tile", "producer_consumer"])
@pytest.mark.parametrize("name", TILE_NAMES)
def test_fused_encoded_blend_at_every_pass_count(orc, dev, name, split):
    """gwbp_blend_scatter_encoded (K = 16) in both of its forms, against the oracle fed the encoded map."""
    c = tile_case(dev, name)
    sc, eng, view = c["sc"], c["eng"], c["view"]
    K, n_out = 16, 3
    fmap = torch.randn(sc["H"], sc["W"], K, device=dev, generator=torch.Generator(device=dev).manual_seed(8))
    enc = torch.randn(K, n_out, generator=torch.Generator().manual_seed(9)).abs() / K
    fmap = fmap.abs_()
    encoded = torch.empty(sc["H"], sc["W"], n_out, device=dev)
    for j in range(n_out):  # (column by column: no [H, W, K] float64 copy of the widest image)
        encoded[..., j] = (fmap * enc[:, j].to(dev)).sum(dim=2, dtype=torch.float64).float()
    F, d = torch.zeros(c["n"], n_out, device=dev), torch.zeros(c["n"], device=dev)
    eng.set_split_encoder(split)
    alphas = eng.blend_scatter_encoded(view, fmap, enc.to(dev), F, d, want_alphas=True)
    eng.set_split_encoder(False)
    st = eng.stats()
    assert st["overflow"] == 0 and st["n_pairs"] == len(fb.pairs(sc)[0])
    assert np.array_equal(_bits(alphas.cpu().numpy()), _bits(fb.pairs(sc)[2]))
    _assert_field(F, d, *_oracle_field(orc, sc, encoded.cpu().numpy()), f"{name} blend_scatter_encoded split={split}")


# ---- B. depth ties ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,image,n_depths", fb.TIE_CASES, ids=fb.TIE_IDS)
def test_depth_ties_keep_ascending_index(orc, dev, n, image, n_depths):
    facts = fb.check_tie_scene(n, image, n_depths)
    sc = fb.tie_scene(n, image, n_depths)
    # (a tile's entries live in ONE of the pool's 32 shards: the images whose single tile holds every pair need 32 x its store)
    caps = {} if image == "small" else dict(pair_cap=1 << 23)
    eng = gsbp_amd.Engine(n, sc["W"], sc["H"], device=dev, **caps)
    view = _front(eng, sc, _on_dev(sc, dev))
    _store_exact(eng, view, sc)
    D = 8
    fmap, fnp = _map(sc, D, dev, seed=2)
    F, d = torch.zeros(n, D, device=dev), torch.zeros(n, device=dev)
    eng.scatter(view, fmap, F, d)
    _assert_field(F, d, *_oracle_field(orc, sc, fnp), f"ties N={n} {image} {facts}")


# ---- C. n_isect on a sort-block boundary -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ample", [False, True], ids=["cap_equals_n_isect", "ample_cap"])
@pytest.mark.parametrize("target", fb.BLOCK_TARGETS)
def test_intersection_count_on_a_sort_block_boundary(orc, dev, target, ample):
    fb.check_block_scene(target)
    sc = fb.block_scene(target)
    n = sc["means"].shape[0]
    eng = gsbp_amd.Engine(n, sc["W"], sc["H"], device=dev, isect_cap=None if ample else target)
    assert ample or eng.isect_cap == target
    view = _front(eng, sc, _on_dev(sc, dev))  # (exact, no overflow)
    _store_exact(eng, view, sc)


# ---- D - F. capacities, and the workspace after an overflow ---------------------------------------------------------------------------------
W, H = ws.W, ws.H
MAX_W, MAX_H = 272, 144   # the workspaces take a recovery view larger than the overflowed one (the token map needs >= 256 x 128)
N_BIG = 13000             # > 12 288: the multi-block depth sort, whose intersection count is k_scan_blocksums'
# bit 2 ("this consumer does not fit the blend") on an EMPTY view: no family reports it -- every blend marks what it left even when it
# stored nothing, so its own consumer fits
MAY_REPORT_MISMATCH = frozenset()
_SEQ = {}


def seq_scene(dev, n):
    """The scene of the sequences file (its N = 3000, or N_BIG Gaussians of the same distribution) with every family's input maps."""
    if n not in _SEQ:
        g_cpu = ws._scene(seed=5 if n == ws.N else 6, n=n)
        _SEQ[n] = dict(n=n, g=[t.to(dev) for t in g_cpu], g_np=[t.numpy() for t in g_cpu], maps={}, fresh={}, oracle={})
    return _SEQ[n]


def _maps_for(sq, dev, w, h):
    if (w, h) not in sq["maps"]:
        m = ws._maps(0, w, h)
        if sq["n"] != ws.N:
            m["colors"] = torch.rand(sq["n"], 3, generator=torch.Generator().manual_seed(12))
        sq["maps"][w, h] = {k: v.to(dev) for k, v in m.items()}
    return sq["maps"][w, h]


# the overflowed view, and the fitting views projected after it (further away: fewer intersections and pairs): another camera, another
# camera AND image size; the short pool of E takes a smaller image
VIEW_FIRST = ("first", W, H, ws.CAM_LARGE)
RECOVERY = [("other_camera", W, H, (2.1, 20.0, 4.0)), ("other_size", MAX_W, MAX_H, (4.0, 40.0, 4.2))]
RECOVERY_POOL = [RECOVERY[0], ("small_size", 120, 70, (4.0, 40.0, 4.0))]


def _camera(spec):
    _, w, h, cam = spec
    return ws._camera(*cam, w, h)


def run_family(eng, name, view, m, fill_f=0.0, fill_d=0.0):
    """ws._run for an engine of any N, with F and d starting from a recognisable content."""
    mode, blend, consume, D = ws.FAMILIES[name]
    F = torch.full((eng.n, max(D, 1)), fill_f, device=eng.device)
    d = torch.full((eng.n,), fill_d, device=eng.device)
    m = dict(m, _F=F, _d=d)
    ws._set_flags(eng, mode)
    out = blend(eng, view, m)
    if consume is not None:
        consume(eng, view, m, F, d)
    st = eng.stats()
    res = {k: v.cpu() for k, v in out.items() if v is not None}
    res.update(F=F.cpu().double().numpy(), d=d.cpu().double().numpy(), stats=st)
    if name in ws.STORING:
        res["pairs"] = ws._sorted_pairs(*eng.dump_pairs(view))
    return res


def fresh_run(dev, sq, name, spec, **caps):
    """Family `name` on view `spec` in a new workspace with ample capacities (cached: nobody writes into it)."""
    key = (name, spec[0], tuple(sorted(caps.items())))
    if key not in sq["fresh"]:
        eng = gsbp_amd.Engine(sq["n"], MAX_W, MAX_H, device=dev, **caps)
        vm, K = _camera(spec)
        view = eng.view(vm, K, spec[1], spec[2])
        ws._front(eng, view, sq["g"])
        sq["fresh"][key] = run_family(eng, name, view, _maps_for(sq, dev, spec[1], spec[2]))
        assert sq["fresh"][key]["stats"]["overflow"] == 0
    return sq["fresh"][key]


def _oracle_count(orc, sq, spec):
    """(proj, bins) of the oracle for view `spec`, cached."""
    if spec[0] not in sq["oracle"]:
        vm, K = _camera(spec)
        g = sq["g_np"]
        proj = orc.project(g[0], g[1], g[2], vm.numpy(), K.numpy(), spec[1], spec[2])
        sq["oracle"][spec[0]] = (proj, orc.bin_sort(proj, spec[1], spec[2]))
    return sq["oracle"][spec[0]]


def _recover(eng, dev, sq, name, spec, **fresh_caps):
    """F: the same workspace projects a fitting view; everything equals that view on a fresh workspace, and the sticky bits are gone."""
    vm, K = _camera(spec)
    view = eng.view(vm, K, spec[1], spec[2])
    ws._front(eng, view, sq["g"])
    assert eng.stats()["overflow"] == 0, "the overflow bits survived gwbp_project"
    res = run_family(eng, name, view, _maps_for(sq, dev, spec[1], spec[2]))
    ref = fresh_run(dev, sq, name, spec, **fresh_caps)
    assert ref["stats"]["n_visible"] > 100 and (name == "render" or ref["stats"]["n_pairs"] > 0)
    ws._assert_same(res, ref, stats=name != "render", what=f"{name}, view {spec[0]} after an overflow")


@pytest.mark.parametrize("n", [ws.N, N_BIG], ids=["sort_small_tail", "scan_blocksums"])
def test_isect_cap_equal_to_the_count_is_exact(orc, dev, n):
    sq = seq_scene(dev, n)
    proj, ref = _oracle_count(orc, sq, VIEW_FIRST)
    cap = ref["n_isect"]
    assert cap > fb.SORT_BLOCK and (n > fb.SMALL_SORT[-1]) == (n == N_BIG)
    eng = gsbp_amd.Engine(n, W, H, device=dev, isect_cap=cap)
    vm, K = _camera(VIEW_FIRST)
    view = eng.view(vm, K, W, H)
    eng.project(view, *sq["g"])
    bins = eng.bin_sort(view, want_outputs=True)
    st = eng.stats()
    assert st["overflow"] == 0 and st["n_isect"] == cap and st["n_visible"] == int((proj["radii"] > 0).sum())
    assert np.array_equal(bins["tile_offsets"].cpu().numpy(), ref["tile_offsets"])
    assert np.array_equal(bins["flatten_ids"].cpu().numpy(), ref["flatten_ids"])  # (the output buffers hold isect_cap entries)
    assert np.array_equal(bins["isect_ids"].cpu().numpy(), ref["isect_ids"])
    alphas = eng.blend_weights(view, want_alphas=True)
    k, w = sort_pairs(*(t.cpu().numpy() for t in eng.dump_pairs(view)))
    g = sq["g_np"]
    rg, rp, rw, ralpha = orc.blend_pairs(proj, ref, g[3], W, H, want_alphas=True)
    rk, rw = sort_pairs(rg, rp, rw)
    assert np.array_equal(k, rk) and np.array_equal(_bits(w), _bits(rw))
    assert np.array_equal(_bits(alphas.cpu().numpy()), _bits(ralpha))


_SHORT = {}


def short_engine(orc, dev, n):
    """One workspace per scene whose isect_cap is ONE less than the first view's intersection count."""
    if n not in _SHORT:
        sq = seq_scene(dev, n)
        cap = _oracle_count(orc, sq, VIEW_FIRST)[1]["n_isect"] - 1
        for spec in RECOVERY:  # (the recovery views fit)
            assert 0 < _oracle_count(orc, sq, spec)[1]["n_isect"] <= cap
        _SHORT[n] = (gsbp_amd.Engine(n, MAX_W, MAX_H, device=dev, isect_cap=cap), cap)
    return _SHORT[n]


@pytest.mark.parametrize("name", list(ws.FAMILIES))
@pytest.mark.parametrize("n", [ws.N, N_BIG], ids=["sort_small_tail", "scan_blocksums"])
def test_isect_cap_one_short_is_an_empty_view_and_the_workspace_recovers(orc, dev, n, name):
    sq = seq_scene(dev, n)
    eng, cap = short_engine(orc, dev, n)
    vm, K = _camera(VIEW_FIRST)
    view = eng.view(vm, K, W, H)
    ws._front(eng, view, sq["g"])
    st = eng.stats()
    assert st["overflow"] == 1 and st["n_isect"] == 0 and st["n_pairs"] == 0, st
    assert st["n_visible"] == int((_oracle_count(orc, sq, VIEW_FIRST)[0]["radii"] > 0).sum())
    res = run_family(eng, name, view, _maps_for(sq, dev, W, H), fill_f=0.5, fill_d=0.25)
    assert (res["F"] == 0.5).all() and (res["d"] == 0.25).all(), f"{name} wrote into F or d on an overflowed view"
    assert not res["alphas"].any(), "alphas of an empty view"
    assert "image" not in res or not res["image"].any(), "the image of an empty view is the background"
    assert "pairs" not in res or len(res["pairs"][0]) == 0
    st = res["stats"]
    allowed = 1 | (4 if name in MAY_REPORT_MISMATCH else 0)
    assert st["overflow"] & 1 and not st["overflow"] & ~allowed, st
    assert st["n_isect"] == 0 and st["n_pairs"] == 0 and st["n_headers"] == 0, st
    _recover(eng, dev, sq, name, RECOVERY[list(ws.FAMILIES).index(name) % 2])


@pytest.mark.parametrize("name", ["w128", "wide256"])
def test_pair_cap_at_pool_used_fits_one_less_overflows_and_the_workspace_recovers(orc, dev, name):
    sq = seq_scene(dev, ws.N)
    ref = fresh_run(dev, sq, name, VIEW_FIRST)
    used = ref["stats"]["pool_used"]
    assert used > 0 and used % (32 * 1024) == 0  # kShards x (pages of the fullest shard) x kPage
    m = _maps_for(sq, dev, W, H)
    vm, K = _camera(VIEW_FIRST)
    # pair_cap == pool_used: every shard's capacity is the fullest shard's need
    eng = gsbp_amd.Engine(ws.N, MAX_W, MAX_H, device=dev, pair_cap=used)
    view = eng.view(vm, K, W, H)
    ws._front(eng, view, sq["g"])
    ws._assert_same(run_family(eng, name, view, m), ref, what=f"{name} at pair_cap == pool_used")
    # one entry less: shard_cap = (pair_cap / 32) & ~1023 loses a page, the fullest shard's last page does not fit
    eng = gsbp_amd.Engine(ws.N, MAX_W, MAX_H, device=dev, pair_cap=used - 1)
    shard_cap = ((used - 1) // 32) & ~1023
    for spec in RECOVERY_POOL:
        ample = fresh_run(dev, sq, name, spec)
        assert 0 < ample["stats"]["pool_used"] <= 32 * shard_cap, "the recovery view does not fit the short pool"
        view = eng.view(vm, K, W, H)
        ws._front(eng, view, sq["g"])
        ws._set_flags(eng, ws.FAMILIES[name][0])
        alphas = ws.FAMILIES[name][1](eng, view, m)["alphas"]  # (the blend alone: the store of this view is invalid)
        st = eng.stats()
        assert st["overflow"] == 2, st
        assert (st["n_isect"], st["n_visible"]) == (ref["stats"]["n_isect"], ref["stats"]["n_visible"])
        # the pair counter keeps counting when the pool is exhausted (include/gwbp.h; Engine.grow sizes the retry from it)
        assert st["n_pairs"] == ref["stats"]["n_pairs"], (st, ref["stats"])
        assert torch.equal(alphas.cpu(), ref["alphas"])  # (the blend itself is complete; only the store is not)
        _recover(eng, dev, sq, name, spec)
