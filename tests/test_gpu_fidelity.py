"""The field comparison on the GPU (gwbp_field_compare, gsbp_amd.fidelity): the five sums against float64 sums of the library's own
render within the worst-case rounding of an fp32 sum, against the numpy reference on the oracle, every map form against the
contiguous fp32 map, the edge cases, reproducibility, memory, and the loop it exists for: agreement -> weights -> a better lift.
Scene, seeds and the reference: tests/fidelity_ref.py."""
import numpy as np
import pytest
import torch

import gsbp_amd
from gsbp_amd.rasterization import get_engine

import fidelity_ref as ref

pytestmark = pytest.mark.gpu
W, H, N = ref.W, ref.H, ref.N
DIMS = (8, 132, 256, 516, 1024)  # both walks, a partial last block, two and four blocks
U = 2.0 ** -24
_CTX = {}


def ctx(dev):
    """The scene on the device and an engine of its own with view 0 projected, sorted and blended."""
    if not _CTX:
        gauss, vms, K = ref.scene()
        gauss, vms, K = tuple(t.to(dev) for t in gauss), vms.to(dev), K.to(dev)
        eng = gsbp_amd.Engine(N, W, H, device=dev)
        view = eng.view(vms[0], K, W, H)
        eng.project(view, *gauss)
        eng.bin_sort(view)
        alphas = eng.blend_weights(view, want_alphas=True)
        assert not eng.stats()["overflow"]
        _CTX.update(gauss=gauss, vms=vms, K=K, eng=eng, view=view, alphas=alphas, fields={}, maps={})
    return _CTX


def field_of(dev, dim):
    """The field lifted from the four views' maps (shared: nobody writes into it) and the maps on the device."""
    c = ctx(dev)
    if dim not in c["fields"]:
        maps = [ref.feature_map(v, dim).to(dev) for v in range(ref.N_VIEWS)]
        c["maps"][dim] = maps
        c["fields"][dim] = gsbp_amd.create_feature_field(*c["gauss"], c["vms"], c["K"], W, H, lambda v: maps[v], dim)
    return c["fields"][dim], c["maps"][dim]


def sums64(r, m):
    """(five float64 [H, W] sums, their per-pixel sums of |term|) of a render r and a map m on the device."""
    r, m = r.double(), m.double()
    d = r - m
    terms = dict(dot=r * m, rr=r * r, mm=m * m, l1=d.abs(), l2=d * d)
    return {k: t.sum(-1) for k, t in terms.items()}, {k: t.abs().sum(-1) for k, t in terms.items()}


def assert_within_rounding(planes, want, scale, dim, what):
    for i, k in enumerate(ref.NAMES):
        err = (planes[i].double() - want[k]).abs()
        bound = (dim + 2) * U * scale[k]
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"{what} D={dim} {k}: max |err| = {float(err.max()):.3e}, max err / bound = {worst:.3f}")
        assert bool((err <= bound).all()), (what, dim, k, worst)


# ---- 1. against the library's own render --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
def test_sums_equal_float64_sums_of_the_librarys_render(dev, dim):
    c = ctx(dev)
    field, maps = field_of(dev, dim)
    r = c["eng"].render(c["view"], field)
    planes, table = c["eng"].field_compare(c["view"], field, maps[0])
    assert planes.shape == (6, H, W) and planes.dtype == torch.float32 and table.shape == (8,) and table.dtype == torch.float64
    want, scale = sums64(r, maps[0])
    assert_within_rounding(planes, want, scale, dim, "render")
    cos = want["dot"] / (want["rr"] * want["mm"]).sqrt()
    live = (want["rr"] * want["mm"]) > 0
    # the cosine inherits the bounds of its three sums (first order), plus its own rounding to fp32
    cos_bound = (dim + 2) * U * (scale["dot"] / (want["rr"] * want["mm"]).sqrt() + cos.abs()) + 2.0 ** -23
    assert bool(((planes[5].double() - cos).abs() <= cos_bound)[live].all()) and bool(torch.isnan(planes[5][~live]).all())
    valid = torch.isfinite(planes[:5]).all(0) & (planes[1] > 0) & (planes[2] > 0)
    t = table.cpu().numpy()
    assert t[4] == int(valid.sum()) and t[5] == 0 and t[6] == H * W and t[7] == dim and t[4] > 0.9 * H * W
    for col, i in ((0, 5), (1, 3), (2, 4), (3, 2)):
        assert t[col] == pytest.approx(float(planes[i][valid].double().sum()), rel=1e-12)
    # through the public call: the same planes, and the render's alpha bit for bit
    out = gsbp_amd.render_field_agreement(*c["gauss"], field, maps[0], c["vms"][0], c["K"], W, H)
    assert set(out) == {"dot", "rr", "mm", "l1", "l2", "cosine", "alpha"}
    assert all(torch.equal(out[k], planes[i]) or k == "cosine" for i, k in enumerate(ref.NAMES))
    assert torch.equal(torch.nan_to_num(out["cosine"], nan=7.0), torch.nan_to_num(planes[5], nan=7.0))
    assert torch.equal(out["alpha"], c["alphas"])
    if dim > 16:  # (narrower tables are rendered pixel-parallel by rasterization(), without the weight store)
        _, alpha_r, _ = gsbp_amd.rasterization(*c["gauss"], field, c["vms"][:1], c["K"][None], W, H, want_meta=False)
        assert torch.equal(out["alpha"], alpha_r[0, ..., 0])


# ---- 2. against the CPU reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", (32, 256))
def test_planes_match_the_numpy_reference_on_the_oracle(dev, orc, dim):
    c = ctx(dev)
    field, maps = field_of(dev, dim)
    f_host, m_host = field.cpu().numpy(), maps[0].cpu().numpy()
    sens = ref.sensitive(0, f_host, m_host)
    cap = int(0.005 * H * W)
    print(f"D={dim}: {int(sens.sum())} sensitive pixels in the reference (cap {cap})")
    assert int(sens.sum()) <= cap  # before the kernel's output is looked at
    want, scale = ref.reference(0, f_host, m_host)
    planes, table = c["eng"].field_compare(c["view"], field, maps[0])
    got = planes.cpu().numpy().astype(np.float64)
    over = np.zeros((H, W), bool)
    for i, k in enumerate(ref.NAMES):
        err = np.abs(got[i] - want[k])
        print(f"D={dim} {k}: max |err| / scale = {float((err / np.maximum(scale[k], 1e-30)).max()):.3e}")
        over |= err > ref.TOL * scale[k]
    print(f"D={dim}: {int(over.sum())} pixels beyond {ref.TOL} relative")
    assert int(over.sum()) <= cap
    assert np.abs(c["alphas"].cpu().numpy() - ref.pairs(0)[3]).max() <= ref.TOL
    keep = ~over & want["valid"]
    assert np.abs(got[5] - want["cosine"])[keep].max() <= 1e-4
    t, tw = table.cpu().numpy(), ref.table_of(want, dim)
    assert t[4] == tw[4] and t[5] == 0 and np.allclose(t[:4], tw[:4], rtol=1e-3)


# ---- 3. map forms -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", (8, 256, 516))
def test_map_forms_equal_the_contiguous_fp32_map(dev, dim):
    c = ctx(dev)
    eng, view = c["eng"], c["view"]
    field, maps = field_of(dev, dim)
    m = maps[0]
    base, base_t = eng.field_compare(view, field, m)

    def same(a, b):
        return torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0))
    for dt in (torch.float16, torch.bfloat16):
        half = m.to(dt)
        got, got_t = eng.field_compare(view, field, half)
        ref_p, ref_t = eng.field_compare(view, field, half.float())
        assert same(got, ref_p) and torch.equal(got_t, ref_t), dt
        want, scale = sums64(eng.render(view, field), half.float())
        assert_within_rounding(got, want, scale, dim, str(dt))
    # a padded row stride (and pixel stride): the view of a wider buffer, 16-B aligned or not
    for pad in (4, 3):
        wide = torch.zeros(H, W + 2, dim + pad, device=dev)
        wide[:, :W, :dim] = m
        got, got_t = eng.field_compare(view, field, wide[:, :W, :dim])
        assert same(got, base) and torch.equal(got_t, base_t), pad
    # a field with a padded row stride is read in place
    fw = torch.zeros(N, dim + 4, device=dev)
    fw[:, :dim] = field
    got, got_t = eng.field_compare(view, fw[:, :dim], m)
    assert same(got, base) and torch.equal(got_t, base_t)
    # a 5 x 7 low-resolution map, nearest, against the expanded map
    low = torch.nn.functional.normalize(torch.randn(5, 7, dim, generator=torch.Generator().manual_seed(3)), dim=-1).to(dev)
    up = torch.nn.functional.interpolate(low.permute(2, 0, 1)[None], size=(H, W), mode="nearest")[0].permute(1, 2, 0).contiguous()
    got, got_t = eng.field_compare(view, field, low, index=eng.nearest_maps(5, 7, H, W))
    exp_p, exp_t = eng.field_compare(view, field, up)
    assert same(got, exp_p) and torch.equal(got_t, exp_t)
    out = gsbp_amd.render_field_agreement(*c["gauss"], field, low, c["vms"][0], c["K"], W, H, upsample="nearest")
    assert torch.equal(out["l2"], exp_p[4])
    with pytest.raises(gsbp_amd.GwbpError, match="upsampled"):
        gsbp_amd.render_field_agreement(*c["gauss"], field, low, c["vms"][0], c["K"], W, H, upsample="bilinear")


# ---- 4. edge cases ------------------------------------------------------------------------------------------------------------------
def test_a_view_that_sees_nothing_a_nan_and_an_inf_pixel_and_no_gaussians(dev):
    c = ctx(dev)
    dim = 132
    field, maps = field_of(dev, dim)
    away = c["vms"][0].clone()
    away[:3, :3] = away[:3, :3] * torch.tensor([[1.0], [-1.0], [-1.0]], device=dev)  # turned round: the scene lies behind the camera
    away[:3, 3] = away[:3, 3] * torch.tensor([1.0, -1.0, -1.0], device=dev)
    out = gsbp_amd.render_field_agreement(*c["gauss"], field, maps[0], away, c["K"], W, H)
    assert float(out["alpha"].abs().max()) == 0.0
    assert float(out["rr"].abs().max()) == 0.0 and float(out["dot"].abs().max()) == 0.0
    assert torch.equal(out["l2"], out["mm"]) and bool(torch.isnan(out["cosine"]).all())
    table = gsbp_amd.score_field_views(*c["gauss"], field, away[None], c["K"], W, H, lambda v: maps[0])
    assert table[0].tolist() == [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, float(H * W), float(dim)]
    rep = gsbp_amd.field_fidelity(table)
    assert rep["views_scored"] == 0 and np.isnan(rep["overall"]["cosine"]) and bool(torch.isnan(rep["per_view"]["mse"]).all())
    # one NaN and one Inf pixel
    eng, view = c["eng"], c["view"]
    base, base_t = eng.field_compare(view, field, maps[0])
    m = maps[0].clone()
    m[3, 5, 7], m[40, 69, dim - 1] = float("nan"), float("inf")
    got, got_t = eng.field_compare(view, field, m)
    hit = torch.zeros(H, W, dtype=torch.bool, device=dev)
    hit[3, 5] = hit[40, 69] = True
    assert torch.equal(torch.nan_to_num(got[:, ~hit], nan=7.0), torch.nan_to_num(base[:, ~hit], nan=7.0))
    assert bool(torch.isnan(got[:, hit]).all())
    assert float(got_t[5]) == 2.0 and float(got_t[4]) == float(base_t[4]) - 2.0
    # N = 0
    z3, z4, z1 = torch.zeros(0, 3, device=dev), torch.zeros(0, 4, device=dev), torch.zeros(0, device=dev)
    out = gsbp_amd.render_field_agreement(z3, z4, z3, z1, torch.zeros(0, dim, device=dev), maps[0], c["vms"][0], c["K"], W, H)
    assert float(out["rr"].abs().max()) == 0.0 and torch.equal(out["l2"], out["mm"]) and float(out["alpha"].abs().max()) == 0.0


# ---- 5. reproducibility -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", (132, 1024))
def test_two_calls_and_the_table_only_call_give_the_same_bits(dev, dim):
    c = ctx(dev)
    field, maps = field_of(dev, dim)
    a, at = c["eng"].field_compare(c["view"], field, maps[0])
    b, bt = c["eng"].field_compare(c["view"], field, maps[0])
    none, ct = c["eng"].field_compare(c["view"], field, maps[0], want_planes=False)
    assert none is None
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(at.view(torch.int64), bt.view(torch.int64)) and torch.equal(at.view(torch.int64), ct.view(torch.int64))
    t1 = gsbp_amd.score_field_views(*c["gauss"], field, c["vms"], c["K"], W, H, lambda v: maps[v])
    t2 = gsbp_amd.score_field_views(*c["gauss"], field, c["vms"], c["K"], W, H, lambda v: maps[v])
    assert t1.shape == (ref.N_VIEWS, 8) and torch.equal(t1.view(torch.int64), t2.view(torch.int64))
    assert torch.equal(t1[0].view(torch.int64), at.view(torch.int64))


# ---- 6. memory ----------------------------------------------------------------------------------------------------------------------
def test_scoring_views_allocates_no_image(dev):
    w, h, dim, n = 160, 120, 512, 2000
    cfg = gsbp_amd.synthetic.Config("FID-M", n, 2, w, h, dim, 0.08, False)
    gauss = tuple(t.to(dev).contiguous() for t in gsbp_amd.synthetic.activate(gsbp_amd.synthetic.make_scene(cfg, seed=ref.SEED)))
    vms, K = gsbp_amd.synthetic.make_cameras(cfg).to(dev), gsbp_amd.synthetic.intrinsics(cfg).to(dev)
    maps = [gsbp_amd.synthetic.make_feature_map(cfg, v, device=dev) for v in range(2)]
    field = torch.nn.functional.normalize(torch.randn(n, dim, generator=torch.Generator().manual_seed(1)), dim=1).to(dev)
    get_engine(dev, n, w, h)  # the engine is built
    gsbp_amd.score_field_views(*gauss, field, vms[:1], K, w, h, lambda v: maps[v])  # ... and has its capacities
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    table = gsbp_amd.score_field_views(*gauss, field, vms, K, w, h, lambda v: maps[v])
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"score_field_views on two {w} x {h} x {dim} views: peak memory rose by {rise} bytes; 64 H W = {64 * h * w}, the "
          f"literal form's render alone 4 H W D = {4 * h * w * dim}")
    assert rise < 64 * h * w
    assert float(table[:, 4].min()) > 0


# ---- 7. the loop it exists for ------------------------------------------------------------------------------------------------------
def test_agreement_weights_find_a_corrupted_block_and_the_second_lift_is_better(dev, orc):
    """The four views' maps here are fidelity_ref.consistent_maps -- renders of one seeded truth field -- not
    synthetic.make_feature_map's: those draw every pixel independently, no field can agree with them (the reference alone zeroes
    98.9 % of the covered pixels outside the block at cosine_min = 0.5, see consistent_maps), and the shares asked for below are
    about a field that agrees with its maps except where one of them was spoilt."""
    c = ctx(dev)
    dim = 32
    clean = [torch.from_numpy(m.copy()).to(dev) for m in ref.consistent_maps(dim)]
    y0, y1, x0, x1 = ref.block_of_view2()
    dirty2 = torch.from_numpy(ref.corrupt(clean[2].cpu().numpy())).to(dev)
    maps = [clean[0], clean[1], dirty2, clean[3]]
    first = gsbp_amd.create_feature_field(*c["gauss"], c["vms"], c["K"], W, H, lambda v: maps[v], dim)
    block = np.zeros((H, W), bool)
    block[y0:y1, x0:x1] = True

    def shares(cosine, alpha):
        zeroed = ~(np.isfinite(cosine) & (cosine >= 0.5))
        seen = alpha > 0.5
        return (zeroed & block & seen).sum() / max(1, (block & seen).sum()), (zeroed & ~block & seen).sum() / max(1, (~block & seen).sum())
    # the reference alone meets both shares for this seed
    want, _ = ref.reference(2, first.cpu().numpy(), dirty2.cpu().numpy())
    r_in, r_out = shares(want["cosine"], ref.pairs(2)[3])
    print(f"reference: {r_in:.3f} of the block zeroed, {r_out:.3f} outside")
    assert r_in >= 0.9 and r_out <= 0.05
    planes = gsbp_amd.render_field_agreement(*c["gauss"], first, maps[2], c["vms"][2], c["K"], W, H)
    weight2 = gsbp_amd.agreement_weights(planes, cosine_min=0.5)
    assert weight2.dtype == torch.bool and weight2.shape == (H, W)
    g_in, g_out = shares(planes["cosine"].cpu().numpy(), planes["alpha"].cpu().numpy())
    print(f"kernel: {g_in:.3f} of the block zeroed, {g_out:.3f} outside")
    assert g_in >= 0.9 and g_out <= 0.05
    # view 2 is lifted again with its agreement as weights; the other views count in full
    ones = torch.ones(H, W, dtype=torch.bool, device=dev)
    second = gsbp_amd.create_feature_field(*c["gauss"], c["vms"], c["K"], W, H, lambda v: maps[v], dim,
                                           pixel_weight_fn=lambda v: weight2 if v == 2 else ones)
    score = [gsbp_amd.field_fidelity(gsbp_amd.score_field_views(*c["gauss"], f, c["vms"], c["K"], W, H, lambda v: clean[v]))
             for f in (first, second)]
    print(f"overall mean cosine against the clean maps: first lift {score[0]['overall']['cosine']:.6f}, "
          f"second {score[1]['overall']['cosine']:.6f}")
    assert score[1]["overall"]["cosine"] > score[0]["overall"]["cosine"]


# ---- argument errors ----------------------------------------------------------------------------------------------------------------
def test_argument_errors_raise_and_leave_the_device_usable(dev):
    c = ctx(dev)
    eng, view = c["eng"], c["view"]
    field, maps = field_of(dev, 8)
    for args, kw, msg in (((field[:-1], maps[0]), {}, "rows"), ((field.double(), maps[0]), {}, "float32"),
                          ((field, maps[0][:-1]), {}, r"\[H,W,D\]"), ((field, maps[0][..., :4]), {}, "D = 8"),
                          ((field, maps[0].double()), {}, "float32, float16 or bfloat16"),
                          ((field, maps[0].permute(2, 0, 1).contiguous().permute(1, 2, 0)), {}, "contiguous"),
                          ((field, maps[0]), dict(index=(torch.zeros(H, dtype=torch.int32, device=dev), None)), "index"),
                          ((field, maps[0]), dict(table=torch.zeros(8, device=dev)), "float64")):
        with pytest.raises(gsbp_amd.GwbpError, match=msg):
            eng.field_compare(view, *args, **kw)
    with pytest.raises(TypeError):
        gsbp_amd.render_field_agreement(*c["gauss"], field, maps[0], c["vms"][0], c["K"], W, H, sh_degree=3)
    again, _ = eng.field_compare(view, field, maps[0])
    assert bool(torch.isfinite(again[:5]).all())
