"""Call sequences on a reused workspace.  Every other parity test runs project, bin_sort, one blend and one consumer and then
re-projects or drops the engine, and gwbp_project's memset hides whatever device state a blend or a consumer leaves behind.
The C ABI allows more: a consumer read twice from one weight store, a projected view blended again (another weight map, the
driver's token fallback), one workspace for views of any size.  Here the reference of every blend / consumer family is its
result on a FRESH workspace (pinned once against the CPU oracle at the top), and the sequences must reproduce it: stats, pairs,
alphas and images bit for bit, F and d up to the order of the atomic sums."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from util import rel_row_err

import gsbp_amd

pytestmark = pytest.mark.gpu

N, W, H = 3000, 257, 131  # 17 x 9 tiles: every XCD class of the scatter queues owns tiles, edge tiles on both axes
LR_H, LR_W = 8, 16         # token map: texels at least a tile wide and high at 257 x 131
K_ENC, N_OUT = 64, 16      # encoder of the compressed variant
N_CLASSES, N_MASKS = 7, 4  # label map: classes 0..6 (7 never appears: an empty column); mask table of 4 rows
EXACT_KEYS = ("n_pairs", "n_isect", "n_visible", "n_headers", "pool_used", "blend_kind")


def _scene(seed=5, n=N, log_scale0=0.03):
    g = torch.Generator().manual_seed(4100 + seed)
    means = torch.rand(n, 3, generator=g) * 2.0 - 1.0
    scales = torch.exp(math.log(log_scale0) + 0.7 * torch.randn(n, 3, generator=g))
    quats = torch.randn(n, 4, generator=g)
    opac = torch.sigmoid(2.0 * torch.randn(n, generator=g))
    return means, quats, scales, opac


def _camera(th, el_deg, r, w, h, zoom=1.0, away=False):
    el = math.radians(el_deg)
    c = torch.tensor([r * math.cos(th) * math.cos(el), r * math.sin(th) * math.cos(el), r * math.sin(el)])
    fwd = c / c.norm() if away else -c / c.norm()  # away: the scene lies behind the camera, everything is culled
    right = torch.linalg.cross(fwd, torch.tensor([0.0, 0.0, 1.0]))
    right = right / right.norm()
    down = torch.linalg.cross(fwd, right)
    R = torch.stack([right, down, fwd])
    vm = torch.eye(4)
    vm[:3, :3] = R
    vm[:3, 3] = -R @ c
    f = 0.9 * w * zoom
    K = torch.tensor([[f, 0, w / 2 + 1.3], [0, 0.95 * f, h / 2 - 0.7], [0, 0, 1.0]])
    return vm, K


CAM_LARGE = (0.7, 30.0, 3.2)


def _maps(seed, w, h):
    """Every input map of one view, on the CPU (float32 unless stated)."""
    g = torch.Generator().manual_seed(7000 + seed)
    f = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return dict(
        f128=f(h, w, 128), f40=f(h, w, 40), f130=f(h, w, 130), f256=f(h, w, 256), f16=f(h, w, 16), f32=f(h, w, 32),
        k64=f(h, w, K_ENC), enc=f(K_ENC, N_OUT) / 8.0, low=f(11, 23, 128), tok=f(LR_H, LR_W, 128),
        labels=torch.randint(0, N_CLASSES - 1, (h, w), generator=g, dtype=torch.int32),
        mlabels=torch.randint(0, N_MASKS, (h, w), generator=g, dtype=torch.int32),  # <= 4 distinct per record: no spills
        table=f(N_MASKS, 32), mask=torch.rand(h, w, generator=g) > 0.3, colors=torch.rand(N, 3, generator=g))


# ---- the families: (flags, blend, consumer, F width) -----------------------------------------------------------------------
# blend(eng, view, m) -> dict of outputs it makes (alphas, image); consume(eng, view, m, F, d) adds to F and d.  A family
# with consume = None does its whole work in the blend (the fused blends) or makes no weight store at all (render_pixels).
def _b_store(eng, view, m):
    return dict(alphas=eng.blend_weights(view, want_alphas=True))


def _b_store_d(eng, view, m):  # gwbp_blend_weights_d: the denominators inside the blend
    return dict(alphas=eng.blend_weights(view, want_alphas=True, d=m["_d"]))


def _b_tokens(eng, view, m):
    return dict(alphas=eng.blend_tokens(view, LR_H, LR_W, want_alphas=True))


def _b_masked(eng, view, m):
    return dict(alphas=eng.blend_weighted(view, m["mask"], want_alphas=True))


def _b_tokens_masked(eng, view, m):
    return dict(alphas=eng.blend_tokens_weighted(view, LR_H, LR_W, m["mask"], want_alphas=True))


def _b_rgb(eng, view, m):
    image, alphas = eng.blend_weights_rgb(view, m["colors"], want_alphas=True)
    return dict(alphas=alphas, image=image)


def _b_tokens_rgb(eng, view, m):
    image, alphas = eng.blend_tokens_rgb(view, LR_H, LR_W, m["colors"], want_alphas=True)
    return dict(alphas=alphas, image=image)


def _b_render(eng, view, m):
    image, alphas = eng.render_pixels(view, m["colors"])
    return dict(alphas=alphas, image=image)


def _fused(kind, masked=False):
    def blend(eng, view, m):
        F, d = m["_F"], m["_d"]
        if kind == "enc":
            if masked:
                return dict(alphas=eng.blend_scatter_encoded_weighted(view, m["k64"], m["enc"], m["mask"], F, d, want_alphas=True))
            return dict(alphas=eng.blend_scatter_encoded(view, m["k64"], m["enc"], F, d, want_alphas=True))
        if masked:
            return dict(alphas=eng.blend_scatter_weighted(view, m[kind], m["mask"], F, d, want_alphas=True))
        return dict(alphas=eng.blend_scatter(view, m[kind], F, d, want_alphas=True))
    return blend


def _c_scatter(key, upsample=None, dtype=None):
    def consume(eng, view, m, F, d):
        x = m[key] if dtype is None else m[key].to(dtype)
        eng.scatter(view, x, F, d, upsample=upsample)
    return consume


def _c_wide_accd(eng, view, m, F, d):  # the 256-channel scatter without d, then gwbp_accumulate_d
    eng.scatter(view, m["f256"], F, None)
    eng.accumulate_d(view, d)


def _c_wide_nod(eng, view, m, F, d):  # blend_weights_d added d already
    eng.scatter(view, m["f256"], F, None)


def _c_encoded(eng, view, m, F, d):
    eng.scatter_encoded(view, m["k64"], m["enc"], F, d)


def _c_tokens(eng, view, m, F, d):
    eng.scatter_tokens(view, m["tok"], F, d)


def _c_labels(eng, view, m, F, d):
    eng.scatter_labels(view, m["labels"], F, d, N_CLASSES)


def _c_masks(eng, view, m, F, d):
    eng.scatter_mask_features(view, m["mlabels"], m["table"], F, d)


NARROW, WIDE, SPLIT = "narrow", "wide", "split"
FAMILIES = {
    "w128": (NARROW, _b_store, _c_scatter("f128"), 128),
    "w40": (NARROW, _b_store, _c_scatter("f40"), 40),
    "w130": (NARROW, _b_store, _c_scatter("f130"), 130),
    "wide256": (WIDE, _b_store, _c_scatter("f256"), 256),
    "wide_accd": (WIDE, _b_store, _c_wide_accd, 256),
    "wide_blend_d": (WIDE, _b_store_d, _c_wide_nod, 256),
    "nearest": (NARROW, _b_store, _c_scatter("low", "nearest"), 128),
    "bilinear": (NARROW, _b_store, _c_scatter("low", "bilinear"), 128),
    "fp16": (NARROW, _b_store, _c_scatter("f128", dtype=torch.float16), 128),
    "bf16": (NARROW, _b_store, _c_scatter("f128", dtype=torch.bfloat16), 128),
    "encoded": (NARROW, _b_store, _c_encoded, N_OUT),
    "fused16": (NARROW, _fused("f16"), None, 16),
    "fused32": (NARROW, _fused("f32"), None, 32),
    "fused_enc": (NARROW, _fused("enc"), None, N_OUT),
    "fused_split": (SPLIT, _fused("enc"), None, N_OUT),
    "tokens": (NARROW, _b_tokens, _c_tokens, 128),
    "labels": (NARROW, _b_store, _c_labels, N_CLASSES),
    "masks": (NARROW, _b_store, _c_masks, 32),
    "ex_w128": (NARROW, _b_masked, _c_scatter("f128"), 128),
    "ex_fused16": (NARROW, _fused("f16", masked=True), None, 16),
    "ex_split": (SPLIT, _fused("enc", masked=True), None, N_OUT),
    "ex_tokens": (NARROW, _b_tokens_masked, _c_tokens, 128),
    "rgb_w128": (NARROW, _b_rgb, _c_scatter("f128"), 128),
    "rgb_tokens": (NARROW, _b_tokens_rgb, _c_tokens, 128),
    "render": (NARROW, _b_render, None, 0),
}
STORING = {k for k, (_, b, _, _) in FAMILIES.items() if b in (_b_store, _b_store_d, _b_masked, _b_rgb)}
CONSUMED = [k for k, (_, b, c, _) in FAMILIES.items() if c is not None and b is not _b_store_d]
# the families whose repeated consumer must double F bit for bit: one read-modify-write per row, no atomics (no spills here)
RMW = {"tokens", "masks", "ex_tokens", "rgb_tokens"}


def _set_flags(eng, mode):
    eng.set_narrow_scatter(mode != WIDE)
    eng.set_split_encoder(mode == SPLIT)


def _front(eng, view, g):
    eng.project(view, *g)
    eng.bin_sort(view)


def _blend(eng, name, view, m):
    mode, blend, _, _ = FAMILIES[name]
    _set_flags(eng, mode)
    return blend(eng, view, m)


def _run(eng, name, view, m, consumers=1):
    """Blend + consumer(s) of family `name` on the projected view in eng: its outputs, F, d (float64 numpy) and stats."""
    mode, blend, consume, D = FAMILIES[name]
    F = torch.zeros(N, max(D, 1), device=eng.device)
    d = torch.zeros(N, device=eng.device)
    m["_F"], m["_d"] = F, d
    _set_flags(eng, mode)
    out = blend(eng, view, m)
    for _ in range(consumers if consume is not None else 0):
        consume(eng, view, m, F, d)
    st = eng.stats()
    res = {k: v.cpu() for k, v in out.items() if v is not None}
    res.update(F=F.cpu().double().numpy(), d=d.cpu().double().numpy(), stats=st)
    if name in STORING:
        gid, pix, w = eng.dump_pairs(view)
        res["pairs"] = _sorted_pairs(gid, pix, w)
    return res


def _sorted_pairs(gid, pix, w):
    key = gid.cpu().numpy().astype(np.int64) * (1 << 32) + pix.cpu().numpy().astype(np.int64)
    o = np.argsort(key, kind="stable")
    return key[o], w.cpu().numpy()[o]


def _assert_same(res, ref, factor=1, tol=1e-5, stats=True, what=""):
    """res equals ref (a fresh run) with F, d = factor x ref's; bit for bit where no atomics are involved."""
    for k in ("alphas", "image"):
        if k in ref:
            assert torch.equal(res[k], ref[k]), f"{what}: {k} differs from the fresh run"
    if "pairs" in ref:
        assert np.array_equal(res["pairs"][0], ref["pairs"][0]), f"{what}: weight-store pairs differ"
        assert np.array_equal(res["pairs"][1], ref["pairs"][1]), f"{what}: weight-store weights differ"
    if ref["F"].size and np.abs(ref["F"]).max() > 0:
        assert rel_row_err(res["F"], factor * ref["F"]) <= tol, f"{what}: F is not {factor} x fresh"
    if ref["d"].max() > 0:
        assert rel_row_err(res["d"][:, None], factor * ref["d"][:, None]) <= tol, f"{what}: d is not {factor} x fresh"
    else:
        assert res["d"].max() == 0
    if stats:
        got = {k: res["stats"][k] for k in EXACT_KEYS}
        want = {k: ref["stats"][k] for k in EXACT_KEYS}
        assert got == want, f"{what}: stats {got} != fresh {want}"
        assert res["stats"]["overflow"] == 0, f"{what}: overflow {res['stats']['overflow']}"


# ---- fixtures --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(dev):
    g_cpu = _scene()
    vm, K = _camera(*CAM_LARGE, W, H)
    maps = _maps(0, W, H)
    m = {k: v.to(dev) for k, v in maps.items()}
    return dict(g=[t.to(dev) for t in g_cpu], g_np=[t.numpy() for t in g_cpu], vm=vm, K=K, maps=maps, m=m)


def _fresh(dev, sc, name, w=W, h=H, vm=None, K=None, m=None, **caps):
    eng = gsbp_amd.Engine(N, W, H, device=dev, **caps)
    view = eng.view(sc["vm"] if vm is None else vm, sc["K"] if K is None else K, w, h)
    _front(eng, view, sc["g"])
    res = _run(eng, name, view, dict(sc["m"] if m is None else m))
    del eng
    return res


@pytest.fixture(scope="module")
def fresh(dev, scene):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _fresh(dev, scene, name)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def shared(dev):
    """One engine for the sequence tests: every test starts with gwbp_project of its view, so whatever the previous test left
    in the workspace is part of what is checked."""
    return gsbp_amd.Engine(N, W, H, device=dev)


# ---- 0. the fresh results against the CPU oracle ----------------------------------------------------------------------------
def _oracle_map(name, maps):
    """The full-resolution [H, W, C] map whose oracle back-projection is the family's F (and, in its last column, d when the
    family is weighted by the mask)."""
    up = lambda x, mode: TF.interpolate(x.permute(2, 0, 1)[None], size=(H, W), mode=mode,  # noqa: E731
                                        **({} if mode == "nearest" else dict(align_corners=False)))[0].permute(1, 2, 0)
    enc = lambda: (maps["k64"].double() @ maps["enc"].double()).float()  # noqa: E731
    base = {"w128": maps["f128"], "w40": maps["f40"], "w130": maps["f130"], "wide256": maps["f256"], "wide_accd": maps["f256"],
            "wide_blend_d": maps["f256"], "nearest": None, "bilinear": None, "fp16": maps["f128"].half().float(),
            "bf16": maps["f128"].bfloat16().float(), "fused16": maps["f16"], "fused32": maps["f32"], "ex_w128": maps["f128"],
            "ex_fused16": maps["f16"], "rgb_w128": maps["f128"]}
    if name in base and base[name] is not None:
        f = base[name]
    elif name in ("nearest", "bilinear"):
        f = up(maps["low"], name)
    elif name in ("encoded", "fused_enc", "fused_split", "ex_split"):
        f = enc()
    elif name in ("tokens", "ex_tokens", "rgb_tokens"):
        f = up(maps["tok"], "nearest")
    elif name == "labels":
        f = TF.one_hot(maps["labels"].long(), N_CLASSES).float()
    elif name == "masks":
        f = maps["table"][maps["mlabels"].long()]
    else:
        raise KeyError(name)
    if name.startswith("ex_"):
        c = maps["mask"].float()[..., None]
        f = torch.cat([f * c, c], dim=2)
    return np.ascontiguousarray(f.numpy().astype(np.float32))


@pytest.fixture(scope="module")
def oracle_view(orc, scene):
    g = scene["g_np"]
    vm, K = scene["vm"].numpy(), scene["K"].numpy()
    proj = orc.project(g[0], g[1], g[2], vm, K, W, H)
    bins = orc.bin_sort(proj, W, H)
    _, _, _, alphas = orc.blend_pairs(proj, bins, g[3], W, H, want_alphas=True)
    image, _ = orc.render(proj, bins, g[3], scene["maps"]["colors"].numpy(), W, H)
    return dict(proj=proj, bins=bins, alphas=alphas, image=image)


@pytest.mark.parametrize("name", list(FAMILIES))
def test_fresh_result_matches_the_oracle(name, orc, scene, fresh, oracle_view):
    res = fresh(name)
    st = res["stats"]
    assert st["overflow"] == 0 and st["n_visible"] > 100 and st["n_isect"] == oracle_view["bins"]["n_isect"]
    assert np.abs(res["alphas"].numpy() - oracle_view["alphas"].reshape(H, W)).max() <= 1e-6
    if "image" in res:
        assert np.abs(res["image"].numpy() - oracle_view["image"].reshape(H, W, 3)).max() <= 1e-5
    if name == "render":
        return
    g, vm, K = scene["g_np"], scene["vm"].numpy(), scene["K"].numpy()
    f = _oracle_map(name, scene["maps"])
    Fr = np.zeros((N, f.shape[2]), np.float64)
    dr = np.zeros(N, np.float64)
    info = orc.backproject_view(*g, vm, K, W, H, f, Fr, dr)
    if name.startswith("ex_"):
        Fr, dr = Fr[:, :-1], Fr[:, -1]
    else:
        assert st["n_pairs"] == info["n_pairs"]  # (a weighted blend counts only the pairs of pixels with c != 0)
    assert dr.max() > 0 and np.abs(Fr).max() > 0
    assert rel_row_err(res["F"], Fr) <= 1e-4
    assert rel_row_err(res["d"][:, None], dr[:, None]) <= 1e-4
    if "pairs" in res and not name.startswith("ex_"):
        assert len(res["pairs"][0]) == info["n_pairs"]


# ---- 1. a consumer repeated on one blend --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CONSUMED)
def test_consumer_twice_on_one_blend_doubles_the_result(name, shared, scene, fresh):
    view = shared.view(scene["vm"], scene["K"], W, H)
    _front(shared, view, scene["g"])
    res = _run(shared, name, view, dict(scene["m"]), consumers=2)
    ref = fresh(name)
    if name in RMW:
        assert np.array_equal(res["F"], 2 * ref["F"]) and np.array_equal(res["d"], 2 * ref["d"])
    _assert_same(res, ref, factor=2, what=f"{name} x2")


# ---- 2. blend + consumer repeated on one projection ----------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FAMILIES))
def test_blend_and_consumer_repeated_on_one_projection(name, shared, scene, fresh):
    view = shared.view(scene["vm"], scene["K"], W, H)
    _front(shared, view, scene["g"])
    ref = fresh(name)
    F = np.zeros_like(ref["F"])
    d = np.zeros_like(ref["d"])
    for k in range(1, 4):
        res = _run(shared, name, view, dict(scene["m"]))
        _assert_same(res, ref, what=f"{name} repeat {k}")
        F, d = F + res["F"], d + res["d"]
    if ref["d"].max() > 0:
        assert rel_row_err(F, 3 * ref["F"]) <= 1e-5 and rel_row_err(d[:, None], 3 * ref["d"][:, None]) <= 1e-5


def test_split_encoder_twice_on_one_projection_adds_twice(shared, scene, fresh):
    """The split form's tile counter must be re-armed by the launch itself: a second gwbp_blend_scatter_encoded under
    GWBP_FLAG_SPLIT_ENCODER on the same projected view adds as much as the first (not nothing)."""
    view = shared.view(scene["vm"], scene["K"], W, H)
    _front(shared, view, scene["g"])
    m = dict(scene["m"])
    F = torch.zeros(N, N_OUT, device=shared.device)
    d = torch.zeros(N, device=shared.device)
    shared.set_narrow_scatter(True)
    shared.set_split_encoder(True)
    for _ in range(2):
        shared.blend_scatter_encoded(view, m["k64"], m["enc"], F, d)
    shared.set_split_encoder(False)
    ref = fresh("fused_split")
    assert shared.stats()["overflow"] == 0
    assert rel_row_err(F.cpu().double().numpy(), 2 * ref["F"]) <= 1e-5
    assert rel_row_err(d.cpu().double().numpy()[:, None], 2 * ref["d"][:, None]) <= 1e-5


@pytest.mark.parametrize("name", ["w128", "wide256"])
def test_storing_blends_reuse_the_pool_of_a_workspace_sized_for_one(name, dev, scene, fresh):
    """pair_cap such that one blend's pool_used fits and two do not: five storing blends of one projection must each leave the
    same store and no overflow (every blend starts from its own pool)."""
    ref = fresh(name)
    cap = ref["stats"]["pool_used"]
    assert cap > 0
    eng = gsbp_amd.Engine(N, W, H, device=dev, pair_cap=cap)
    view = eng.view(scene["vm"], scene["K"], W, H)
    _front(eng, view, scene["g"])
    for k in range(5):
        _assert_same(_run(eng, name, view, dict(scene["m"])), ref, what=f"{name} blend {k + 1} at pair_cap {cap}")


# ---- 3. any family, then any family on the same projection --------------------------------------------------------------
TRANSITIONS = [(x, y) for x in FAMILIES for y in FAMILIES]


@pytest.mark.parametrize("x,y", TRANSITIONS, ids=[f"{x}-then-{y}" for x, y in TRANSITIONS])
def test_family_after_family_on_one_projection(x, y, shared, scene, fresh):
    view = shared.view(scene["vm"], scene["K"], W, H)
    _front(shared, view, scene["g"])
    _run(shared, x, view, dict(scene["m"]))
    res, ref = _run(shared, y, view, dict(scene["m"])), fresh(y)
    _assert_same(res, ref, stats=y != "render", what=f"{y} after {x}")
    if y == "render":  # (it blends nothing: the counts of the blend are x's)
        assert (res["stats"]["n_isect"], res["stats"]["n_visible"]) == (ref["stats"]["n_isect"], ref["stats"]["n_visible"])


# ---- 4. consumers that do not fit the blend, through the C ABI ---------------------------------------------------------
def _consumers(eng, view, m, F, d):
    """Every consumer, called with Engine's Python guards bypassed (as the C-ABI tests of test_gpu_parity.py do): the library
    alone must catch the mismatch.  F holds one accumulator per width."""
    def scatter(x, wide):
        def call():
            eng.set_narrow_scatter(not wide)
            eng.scatter(view, x, F[x.shape[2]], d)
        return call

    return {
        "scatter128": scatter(m["f128"], False),
        "scatter256": scatter(m["f256"], True),
        "accumulate_d": lambda: eng.accumulate_d(view, d),
        "encoded": lambda: eng.scatter_encoded(view, m["k64"], m["enc"], F[N_OUT], d),
        "tokens": lambda: eng.scatter_tokens(view, m["tok"], F[128], d),
        "labels": lambda: eng.scatter_labels(view, m["labels"], F[N_CLASSES], d, N_CLASSES),
        "masks": lambda: eng.scatter_mask_features(view, m["mlabels"], m["table"], F[32], d),
    }


# blend -> the consumers that do not fit it (gwbp.h): a weight store without weight sums, a fused blend (no store), tokens
MISMATCH = {
    "w128": (["scatter256", "accumulate_d", "tokens"], "w128"),
    "wide256": (["tokens"], "wide256"),
    "fused16": (["scatter128", "scatter256", "accumulate_d", "encoded", "tokens", "labels", "masks"], "fused16"),
    "fused_enc": (["scatter128", "scatter256", "accumulate_d", "encoded", "tokens", "labels", "masks"], "fused_enc"),
    "fused_split": (["scatter128", "scatter256", "accumulate_d", "encoded", "tokens", "labels", "masks"], "fused_split"),
    "tokens": (["scatter128", "scatter256", "accumulate_d", "encoded", "labels", "masks"], "tokens"),
}


@pytest.mark.parametrize("blend", list(MISMATCH))
def test_mismatched_consumers_fail_or_add_nothing(blend, shared, scene, fresh):
    view = shared.view(scene["vm"], scene["K"], W, H)
    _front(shared, view, scene["g"])
    m = dict(scene["m"])
    _run(shared, blend, view, m)
    # fresh accumulators with a recognisable content, one per width a consumer writes
    widths = (16, 32, 128, 256, N_CLASSES)
    F = {D: torch.full((N, D), 0.5, device=shared.device) for D in widths}
    d = torch.full((N,), 0.25, device=shared.device)
    calls = _consumers(shared, view, m, F, d)
    # after a blend that leaves no weight store (fused: reserved 2, tokens: reserved 3) a store consumer adding nothing is the
    # documented outcome (gwbp.h); after a storing blend a consumer that does not fit must raise bit 2 or fail
    wrong, no_store = MISMATCH[blend][0], blend.startswith("fused") or blend == "tokens"
    for name in wrong:
        shared._tokens = (LR_H, LR_W) if name == "tokens" else None
        shared._halves = True
        try:
            calls[name]()
            rc = 0
        except gsbp_amd.GwbpError:
            rc = -1
        finally:
            shared._tokens, shared._halves = ((LR_H, LR_W) if blend == "tokens" else None), blend == "wide256"
        st = shared.stats()
        untouched = all(bool((t == 0.5).all()) for t in F.values()) and bool((d == 0.25).all())
        assert untouched, f"{name} after {blend} changed F or d (status {rc})"
        if rc == 0:
            assert (st["overflow"] & 4) or no_store, f"{name} after {blend}: no error and no overflow bit 2"
    sticky = shared.stats()["overflow"]
    assert (sticky & ~4) == 0
    # the fitting blend + consumer on the same projection is still right; overflow bits stay until the next gwbp_project
    res = _run(shared, MISMATCH[blend][1], view, m)
    assert res["stats"]["overflow"] == sticky
    _assert_same(res, fresh(MISMATCH[blend][1]), stats=False, what=f"{blend} after mismatched consumers")
    got = {k: res["stats"][k] for k in EXACT_KEYS}
    assert got == {k: fresh(MISMATCH[blend][1])["stats"][k] for k in EXACT_KEYS}
    _front(shared, view, scene["g"])
    assert shared.stats()["overflow"] == 0


# ---- 5. view after view on one workspace ------------------------------------------------------------------------------
def _views():
    return [("large", W, H, _camera(*CAM_LARGE, W, H)),
            ("small_odd", 40, 23, _camera(2.1, 20.0, 2.8, 40, 23)),
            ("culled", W, H, _camera(*CAM_LARGE, W, H, away=True)),
            ("isect_overflow", W, H, _camera(*CAM_LARGE, W, H, zoom=3.0)),
            ("large_again", W, H, _camera(*CAM_LARGE, W, H))]


@pytest.mark.parametrize("name", ["w128", "fused16", "fused_split", "wide256"])
def test_views_of_any_size_on_one_workspace(name, dev, scene):
    ref_eng = gsbp_amd.Engine(N, W, H, device=dev)
    view = ref_eng.view(scene["vm"], scene["K"], W, H)
    _front(ref_eng, view, scene["g"])
    isect_cap = ref_eng.stats()["n_isect"]  # the large view fits exactly; the zoomed one cannot
    del ref_eng
    eng = gsbp_amd.Engine(N, W, H, device=dev, isect_cap=isect_cap)
    for label, w, h, (vm, K) in _views():
        m = {k: v.to(dev) for k, v in _maps(0, w, h).items()}
        view = eng.view(vm, K, w, h)
        _front(eng, view, scene["g"])
        res = _run(eng, name, view, dict(m))
        ref = _fresh(dev, scene, name, w=w, h=h, vm=vm, K=K, m=dict(m), isect_cap=isect_cap)
        if label == "isect_overflow":  # (results invalid: the counts only)
            assert res["stats"]["overflow"] & 1
            for k in ("overflow", "n_isect", "n_visible"):
                assert res["stats"][k] == ref["stats"][k], k
            continue
        if label == "culled":
            assert res["stats"]["n_visible"] == 0 and res["d"].max() == 0
        _assert_same(res, ref, what=f"{name}, view {label}")


# ---- the driver's token fallback ------------------------------------------------------------------------------------------
def test_driver_token_fallback_reports_each_view_once(dev, scene):
    """ViewPipeline._scatter_on re-blends a view that blend_tokens has blended when its map does not suit token space (here:
    a map of another size than the first view's).  The field must equal that of a run without token space, and so must the
    accumulated pair and record counts -- a re-blend of a projected view must not count its pairs twice."""
    V = 4
    cams = [_camera(0.7 + 0.5 * v, 25.0 + 5 * v, 3.2, W, H) for v in range(V)]
    vms = torch.stack([c[0] for c in cams]).to(dev)
    K = cams[0][1].to(dev)
    g = torch.Generator().manual_seed(99)
    maps = [torch.randn(LR_H if v % 2 == 0 else LR_H - 1, LR_W, 128, generator=g).to(dev) for v in range(V)]

    def field(token_space):
        return gsbp_amd.create_feature_field(*scene["g"], vms, K, W, H, lambda v: maps[v], 128, upsample="nearest",
                                             token_space=token_space, return_partials=True)

    out_t, F_t, d_t, st_t = field(True)
    out_u, F_u, d_u, st_u = field(False)
    assert st_t["overflow"] == 0 and st_u["overflow"] == 0
    assert rel_row_err(F_t.cpu().numpy(), F_u.cpu().numpy()) <= 1e-5
    assert rel_row_err(d_t.cpu().numpy()[:, None], d_u.cpu().numpy()[:, None]) <= 1e-5
    for k in ("n_pairs", "n_headers", "n_isect", "n_visible"):
        assert st_t[k] == st_u[k], (k, st_t[k], st_u[k])
