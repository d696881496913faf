"""Densification on the GPU: meta["means2d"].grad of rasterization(means2d_grad=True) against the float64 blend
yardstick, the four kernels of csrc/densify.hip against tests/densify_ref.py -- bit for bit wherever the arithmetic is the documented
float32 chain -- and one densify round with an optimiser and a carried field.

Tolerances.  means2d.grad is columns 0 and 1 of the blend backward's v_g2d, so it is held to that kernel's rule: per figure, kernel
error <= FACTOR x the float32 reference's (tests/test_gpu_blend_grad.py: FACTOR and the floor rule, imported).  accumulate, plan, parent,
child, the copied rows, scaling - log16 and gather are compared exactly.  A split child's mean is compared exactly with the numpy
restatement and, where the device's expf and the once-rounded exponential differ in the last bit, held to densify_ref.split_bound against
float64; at most half of the split rows may need the bound.
"""
import functools
import math

import numpy as np
import pytest
import torch

import blend_grad_ref as bg
import densify_ref as ref
import gsbp_amd
import raster_grad_ref as rg
from gsbp_amd import rasterization
from gsbp_amd import synthetic as syn
from gsbp_amd.densify import emit, gather_rows, plan
from gsbp_amd.polish import render_splats
from test_gpu_blend_grad import FACTOR
from test_gpu_raster_grad import _stack, _t0
from util import scene_np

pytestmark = pytest.mark.gpu
LOG16 = float(np.float32(math.log(1.6)))


# ---- means2d.grad -----------------------------------------------------------------------------------------------------------------
def _t0_with_culled(view):
    """T0 with four Gaussians at the centre of its first camera and three at the centre of its second: depth 0, rows the projection
    culls (the same scene whichever view is asked for)."""
    s = _t0(view=view)
    _, sc = scene_np("T0")
    means = s["inputs"][0].clone()
    for rows, vm in ((slice(0, 4), sc["vms"][0]), (slice(4, 7), sc["vms"][1])):
        means[rows] = -(vm[:3, :3].T @ vm[:3, 3])
    return dict(s, inputs=(means,) + tuple(s["inputs"][1:]))


M2D_CASES = {"t0": lambda: [_t0_with_culled(0)], "stack": lambda: [_stack(0.02)], "two-cameras": lambda: [_t0_with_culled(0), _t0_with_culled(1)]}


@functools.lru_cache(maxsize=None)
def m2d_reference(name):
    """Per camera of the case: the kernels' records, lists and cut (as tests/test_gpu_blend_grad.py takes them), seeded G and A, and the
    float64 and float32 runs of the blend yardstick.  Computed once, shared, never modified."""
    dev = torch.device("cuda:0")
    out = []
    for c, sc in enumerate(M2D_CASES[name]()):
        g = [t.to(dev, torch.float32).contiguous() for t in sc["inputs"][:4]]
        n, W, H = g[0].shape[0], sc["W"], sc["H"]
        eng = gsbp_amd.Engine(n, W, H, device=dev)
        view = eng.view(sc["vm"], sc["K"], W, H)
        while True:
            proj = eng.project(view, *g, want_outputs=True)
            bins = eng.bin_sort(view, want_outputs=True)
            eng.blend_weights(view)
            st = eng.stats()
            if not st["overflow"]:
                break
            eng.grow(st)
        gid, pix, _ = eng.dump_pairs(view)
        vis = proj["radii"] > 0
        rec = [torch.where(vis.reshape(-1, *[1] * (t.dim() - 1)), t, torch.zeros_like(t)).cpu() for t in (proj["means2d"], proj["conics"], g[3])]
        pl = bg.plan(bins["flatten_ids"][:st["n_isect"]].cpu(), bins["tile_offsets"].cpu(), gid.cpu(), pix.cpu(), W, H, n)
        gen = torch.Generator().manual_seed(31 + c)
        G, A = torch.randn(H, W, 3, generator=gen), torch.randn(H, W, generator=gen)
        colors = sc["inputs"][4]
        truth = bg.blend(torch.float64, pl, *rec, colors, G, A)
        floor = bg.blend(torch.float32, pl, *rec, colors, G, A)
        out.append(dict(sc=sc, G=G, A=A, truth=truth["v_g2d"][:, :2], floor=floor["v_g2d"][:, :2], visible=vis.cpu(),
                        means2d=proj["means2d"].cpu()))
    return out


def _means2d_grad(dev, cams, geometry_grad):
    """rasterization(means2d_grad=True) of the case's cameras in ONE call, loss = sum_c sum(out_c G_c) + sum(alpha_c A_c), backward."""
    sc = cams[0]["sc"]
    ins = [t.to(dev).clone() for t in sc["inputs"]]
    for k, t in enumerate(ins):
        t.requires_grad_(geometry_grad or k == 4)
    vms = torch.stack([c["sc"]["vm"] for c in cams]).to(dev)
    Ks = torch.stack([c["sc"]["K"] for c in cams]).to(dev)
    out, alpha, meta = rasterization(*ins, vms, Ks, sc["W"], sc["H"], means2d_grad=True)
    leaf = meta["means2d"]
    assert leaf.requires_grad and leaf.is_leaf and leaf.dtype == torch.float32 and tuple(leaf.shape) == (len(cams), ins[0].shape[0], 2)
    leaf.retain_grad()  # the gsplat strategy protocol: must not raise
    assert leaf.grad is None
    loss = sum((out[c] * cam["G"].to(dev)).sum() + (alpha[c, ..., 0] * cam["A"].to(dev)).sum() for c, cam in enumerate(cams))
    loss.backward()
    assert tuple(meta["radii"].shape) == (len(cams), ins[0].shape[0]) and meta["radii"].dtype == torch.int32
    return leaf, meta, ins


@pytest.mark.parametrize("geometry_grad", [True, False], ids=["all-leaves", "colours-only"])
@pytest.mark.parametrize("name", list(M2D_CASES))
def test_means2d_grad_against_the_float64_blend(dev, name, geometry_grad):
    cams = m2d_reference(name)
    leaf, meta, ins = _means2d_grad(dev, cams, geometry_grad)
    grad = leaf.grad
    assert grad is not None and tuple(grad.shape) == tuple(leaf.shape) and grad.dtype == torch.float32
    assert (ins[0].grad is not None) == geometry_grad and ins[4].grad is not None
    for c, cam in enumerate(cams):
        got = grad[c].cpu()
        vis = cam["visible"]
        assert torch.equal(meta["radii"][c].cpu() > 0, vis)
        assert torch.equal(leaf.detach()[c].cpu()[vis], cam["means2d"][vis])  # the leaf holds the projected means
        assert not got[~vis].any()                                            # culled rows: exact zeros
        if name != "stack":
            assert int((~vis).sum()) >= 3
        assert float(cam["truth"].abs().max()) > 0
        for k, col in enumerate(("mx", "my")):
            for fig, kernel, floor in zip(("fro", "max"), rg.errors(got[:, k], cam["truth"][:, k]), rg.errors(cam["floor"][:, k], cam["truth"][:, k])):
                print(f"{name} camera {c} {col} {fig}: floor {floor:.2e} kernel {kernel:.2e}")
                assert kernel <= FACTOR * floor, (name, c, col, fig, kernel, floor)
        kernel, floor = bg.row_error(got, cam["truth"]), bg.row_error(cam["floor"], cam["truth"])
        print(f"{name} camera {c} rows: floor {floor:.2e} kernel {kernel:.2e}")
        assert kernel <= FACTOR * floor, (name, c, "row", kernel, floor)


def test_means2d_grad_is_off_by_default_and_under_no_grad(dev):
    sc = _t0()
    ins = [t.to(dev).requires_grad_(True) for t in sc["inputs"]]
    cams = (sc["vm"].to(dev)[None], sc["K"].to(dev)[None], sc["W"], sc["H"])
    _, _, meta = rasterization(*ins, *cams)
    assert not meta["means2d"].requires_grad and meta["means2d"].dim() == 2 and meta["radii"].dim() == 1  # packed, as before
    with torch.no_grad():
        _, _, meta = rasterization(*ins, *cams, means2d_grad=True)
    assert not meta["means2d"].requires_grad and meta["means2d"].dim() == 2
    out, _, meta = rasterization(*ins, *cams, means2d_grad=True)
    assert meta["means2d"].requires_grad and meta["camera_ids"].numel() == int((meta["radii"] > 0).sum())  # the packed keys still build
    assert tuple(meta["means2d"].shape) == (1, ins[0].shape[0], 2) and meta["means2d"].grad is None
    out.sum().backward()
    first = meta["means2d"].grad.clone()
    assert float(first.abs().max()) > 0
    with pytest.raises(NotImplementedError):
        rasterization(*ins, *cams, absgrad=True)
    with pytest.raises(NotImplementedError, match="means2d_grad"):
        rasterization(*ins[:4], torch.rand(ins[0].shape[0], 48, device=dev), *cams, means2d_grad=True)


# ---- accumulate -------------------------------------------------------------------------------------------------------------------
def _bits_equal(got, want):
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


@pytest.mark.parametrize("C_", [1, 3])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4099])
def test_accumulate_bit_for_bit(dev, n, C_):
    r = np.random.default_rng(100 * n + C_)
    v = ref.f32(r.normal(size=(C_, n, 2)) * 1e-4)
    radii = r.integers(0, 3, size=(C_, n)).astype(np.int32)  # visible in some cameras only
    v[0, 0, 1], radii[0, 0] = np.nan, 4                      # a NaN gradient on a visible row
    if n > 1:
        v[0, 1, 0], radii[0, 1] = np.nan, 0                  # ... and one on a culled row, which must not be read into the sum
    W, H = 96, 64
    state = gsbp_amd.DensifyState(n, dev)
    g0, c0 = ref.f32(r.random(n)), ref.f32(r.integers(0, 5, size=n))
    state.grad2d, state.count = torch.from_numpy(g0).to(dev), torch.from_numpy(c0).to(dev)
    leaf = torch.zeros(C_, n, 2, device=dev, requires_grad=True)
    leaf.grad = torch.from_numpy(v).to(dev)
    state.update(dict(means2d=leaf, radii=torch.from_numpy(radii).to(dev), width=W, height=H, n_cameras=C_))
    want_g, want_c = ref.accumulate(g0, c0, v, radii, W / 2.0 * C_, H / 2.0 * C_)
    assert _bits_equal(state.grad2d.cpu().numpy(), want_g) and _bits_equal(state.count.cpu().numpy(), want_c)
    got = state.grad2d.cpu().numpy()
    assert np.isnan(got[0]) and np.isfinite(got[1:]).all()


# ---- plan -------------------------------------------------------------------------------------------------------------------------
def _plan_inputs(n, seed):
    r = np.random.default_rng(seed)
    scaling = ref.f32(math.log(0.05) + 0.7 * r.normal(size=(n, 3)))
    opacity = ref.f32(2.0 * r.normal(size=n))
    count = ref.f32(r.integers(0, 6, size=n))
    grad2d = ref.f32(np.abs(r.normal(size=n)) * 1e-3 * np.maximum(count, 1))
    return grad2d, count, scaling, opacity


def _run_plan(dev, grad2d, count, scaling, opacity, th, prune_big):
    kind, offsets = plan(*(torch.from_numpy(a).to(dev) for a in (grad2d, count, scaling, opacity)), th, prune_big)
    return kind.cpu().numpy(), offsets.cpu().numpy()


# both sides of each level of the scan for the 256-lane workgroup: one workgroup, two; one chunk of 256 workgroup sums, two
@pytest.mark.parametrize("n", [0, 1, 256, 257, 65536, 65537])
def test_plan_equals_the_reference(dev, n):
    assert gsbp_amd._lib.DENSIFY_BLOCK == 256
    grad2d, count, scaling, opacity = _plan_inputs(n, 7 + n)
    m, g = ref.largest_scale(scaling), grad2d / np.maximum(count, 1)
    med = (lambda a: float(np.median(a[:len(a) - 1 + len(a) % 2]))) if n else (lambda a: 0.0)
    th = (med(g), med(m), med(m) + 0.3, float(np.quantile(opacity, 0.2)) if n else 0.0, LOG16)
    if n >= 256:  # values exactly on each threshold, and rows nobody counted
        k = np.arange(0, 240, 6)
        count[k], grad2d[k] = 1.0, np.float32(th[0])
        scaling[k + 1] = np.float32(th[1])
        scaling[k + 2] = np.float32(th[2])
        scaling[k + 3] = np.float32(th[2]) + np.float32(LOG16)
        opacity[k + 4] = np.float32(th[3])
        count[k + 5] = 0.0
    for prune_big in (False, True):
        kind, offsets = _run_plan(dev, grad2d, count, scaling, opacity, th, prune_big)
        want_kind, want_offsets = ref.plan(grad2d, count, scaling, opacity, th, prune_big)
        assert kind.dtype == np.uint8 and offsets.dtype == np.int64 and offsets.shape == (n + 1,)
        assert np.array_equal(kind, want_kind) and np.array_equal(offsets, want_offsets)
        if n >= 256:
            assert set(kind) == {0, 1, 2, 3}
    # all pruned: N' = 0; all split: N' = 2 N
    if n:
        kind, offsets = _run_plan(dev, grad2d, count, scaling, opacity, (th[0], th[1], th[2], math.inf, LOG16), False)
        assert not kind.any() and not offsets.any()
        ones = np.ones(n, np.float32)
        kind, offsets = _run_plan(dev, ones, ones, scaling, opacity, (0.5, -math.inf, math.inf, -math.inf, LOG16), True)
        assert (kind == 3).all() and np.array_equal(offsets, 2 * np.arange(n + 1))


# ---- emit and gather --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _round(n=4099, seed=3):
    """One planned and emitted round on the device with the reference's restatement of it: shared, never modified."""
    dev = torch.device("cuda:0")
    r = np.random.default_rng(seed)
    grad2d, count, scaling, opacity = _plan_inputs(n, seed)
    means, rotation = ref.f32(r.normal(size=(n, 3)) * 2.0), ref.f32(r.normal(size=(n, 4)))
    noise = ref.f32(r.normal(size=(n, 2, 3)))
    m, g = ref.largest_scale(scaling), grad2d / np.maximum(count, 1)
    th = (float(np.median(g)), float(np.median(m)), float(np.median(m)) + 0.3, float(np.quantile(opacity, 0.2)), LOG16)
    t = {k: torch.from_numpy(a).to(dev) for k, a in dict(grad2d=grad2d, count=count, scaling=scaling, opacity=opacity, means=means,
                                                         rotation=rotation, noise=noise).items()}
    kind, offsets = plan(t["grad2d"], t["count"], t["scaling"], t["opacity"], th, True)
    n_out = int(offsets[-1])
    new = emit(kind, offsets, n_out, t["means"], t["scaling"], t["rotation"], t["opacity"], t["noise"], LOG16)
    want_kind, want_offsets = ref.plan(grad2d, count, scaling, opacity, th, True)
    want = ref.emit(want_kind, want_offsets, means, scaling, rotation, opacity, noise, LOG16)
    return dict(dev=t, host=dict(means=means, scaling=scaling, rotation=rotation, opacity=opacity, noise=noise), kind=kind, offsets=offsets,
                new=new, want=want, want_kind=want_kind, n=n, n_out=n_out)


def test_emit(dev):
    R = _round()
    new = {k: v.cpu().numpy() for k, v in R["new"].items()}
    want, h = R["want"], R["host"]
    assert np.array_equal(R["kind"].cpu().numpy(), R["want_kind"]) and R["n_out"] == len(want["parent"]) > R["n"] // 2
    assert np.array_equal(new["parent"], want["parent"]) and new["parent"].dtype == np.int32
    assert np.array_equal(new["child"], want["child"]) and new["child"].dtype == np.uint8
    k = R["want_kind"][want["parent"]]
    copied, sp = (k == ref.KEEP) | (k == ref.CLONE), k == ref.SPLIT
    assert copied.sum() > 100 and (k == ref.CLONE).sum() > 100 and sp.sum() > 100 and set(new["child"][sp]) == {0, 1}
    for name in ("means", "scaling", "rotation", "opacity"):  # kept and cloned rows: the source's bits
        assert _bits_equal(new[name][copied], h[name][want["parent"]][copied])
    assert _bits_equal(new["rotation"], want["rotation"]) and _bits_equal(new["opacity"], want["opacity"])
    assert _bits_equal(new["scaling"], want["scaling"])       # scaling - log16 included
    # split means: the restatement's bits, or -- the device's expf differing from the once-rounded exponential -- inside the bound
    same = (new["means"][sp].view(np.uint32) == want["means"][sp].view(np.uint32)).all(axis=1)
    p, c = want["parent"][sp], want["child"][sp]
    m64 = ref.split_means(h["means"][p], h["scaling"][p], h["rotation"][p], h["noise"][p, c], dtype=np.float64)
    ratio = np.abs(new["means"][sp].astype(np.float64) - m64) / ref.split_bound(h["means"][p], h["scaling"][p], h["noise"][p, c])
    share = 1.0 - same.mean()
    print(f"split rows {sp.sum()}: {same.sum()} bit-equal to the restatement, share on the bound {share:.4f}; "
          f"largest error / bound {ratio.max():.3f}")
    assert ratio.max() <= 1.0
    assert share <= 0.5


@pytest.mark.parametrize("mode", ["copy", "zero_new"])
@pytest.mark.parametrize("w", [1, 3, 45, 512])
def test_gather_equals_indexing(dev, w, mode):
    R = _round()
    n = R["n"]
    g = torch.Generator().manual_seed(w)
    wide = torch.randn(n, w + 5, generator=g).to(dev)
    wide[:, w:] = float("nan")                    # what lies between the rows is not read
    parent, child, kind = R["new"]["parent"], R["new"]["child"], R["kind"]
    want = ref.gather(wide[:, :w].cpu().numpy(), R["want"]["parent"], R["want"]["child"], R["want_kind"], mode)
    for table in (wide[:, :w], wide[:, :w].contiguous()):  # row stride w + 5 and w
        got = gather_rows(table, parent, n, child, kind, mode)
        assert tuple(got.shape) == (R["n_out"], w) and _bits_equal(got.cpu().numpy(), want)
    if mode == "zero_new":
        assert (want == 0).all(axis=1).sum() > 100 and (want != 0).all(axis=1).sum() > 100
    shaped = gather_rows(wide[:, :w].contiguous().reshape(n, w, 1), parent, n, child, kind, mode)  # [N, ...] tensors keep their tail
    assert tuple(shaped.shape) == (R["n_out"], w, 1) and _bits_equal(shaped.reshape(-1, w).cpu().numpy(), want)
    empty = gather_rows(wide[:, :w], parent[:0], n, child[:0], kind, mode)
    assert tuple(empty.shape) == (0, w)


# ---- one round with an optimiser and a carried field -----------------------------------------------------------------------------
def t0_training_setup(dev, stride=2):
    """T0 with seeded colours as the target, every second Gaussian of it as the start (what run_train.py --synthetic T0 builds)."""
    cfg = syn.CONFIGS["T0"]
    full = {k: t.to(dev) for k, t in syn.make_scene(cfg).items()}
    n = full["means"].shape[0]
    gen = torch.Generator().manual_seed(syn.SH_SEED)
    full["features_dc"] = ((torch.rand(n, 1, 3, generator=gen) - 0.5) / 0.28209479177387814).to(dev)
    full["features_rest"] = torch.zeros(n, 0, 3, device=dev)
    K, vms = syn.intrinsics(cfg).to(dev), syn.make_cameras(cfg).to(dev)
    with torch.no_grad():
        images = [render_splats(full, vms[v], K, cfg.width, cfg.height).clamp(0.0, 1.0) for v in range(vms.shape[0])]
    start = {k: t[::stride].contiguous() for k, t in full.items()}
    return cfg, start, K, vms, images


def probe_thresholds(dev, start, K, vms, images, cfg, steps=10):
    """`steps` steps of render -> photometric_loss -> backward -> state.update without an optimiser step; the data then chooses the
    thresholds: grow_grad2d = the median of grad2d / count over the counted rows, prune_opa = the 10th percentile of the opacities."""
    work = {k: t.clone().requires_grad_(True) for k, t in start.items()}
    state = gsbp_amd.DensifyState(work["means"].shape[0], dev)
    for s in range(steps):
        v = s % vms.shape[0]
        image, meta = render_splats(work, vms[v], K, cfg.width, cfg.height, return_meta=True, means2d_grad=True)
        gsbp_amd.photometric_loss(image, images[v]).backward()
        state.update(meta)
    seen = state.count > 0
    grow = float(torch.median((state.grad2d / state.count.clamp_min(1))[seen]))
    opa = float(torch.quantile(torch.sigmoid(start["opacity"]), 0.1))
    return work, state, grow, opa


def test_densify_round_trip(dev):
    cfg, start, K, vms, images = t0_training_setup(dev)
    work, state, grow, opa = probe_thresholds(dev, start, K, vms, images, cfg)
    n = work["means"].shape[0]
    assert int((state.count > 0).sum()) > n // 2 and float(state.count.max()) == 10.0
    dcfg = gsbp_amd.DensifyConfig(grow_grad2d=grow, prune_opa=opa, grow_scale3d=0.06, prune_scale3d=0.25)
    results = []
    for _ in range(2):  # twice from the same state and seed: the same bits
        params = {k: t.detach().clone().requires_grad_(True) for k, t in work.items()}
        opt = torch.optim.Adam([dict(params=[params[k]], lr=1e-3) for k in ("means", "scaling", "rotation", "opacity", "features_dc")], eps=1e-15)
        image = render_splats(params, vms[0], K, cfg.width, cfg.height)
        gsbp_amd.photometric_loss(image, images[0]).backward()
        opt.step()
        moments = {k: {m: opt.state[params[k]][m].clone() for m in ("exp_avg", "exp_avg_sq")} for k in ("means", "opacity", "features_dc")}
        st = gsbp_amd.DensifyState(n, dev)
        st.grad2d, st.count = state.grad2d.clone(), state.count.clone()
        field = torch.randn(n, 8, generator=torch.Generator().manual_seed(5)).to(dev)
        step = dcfg.reset_every + 100  # past the first reset: the size criterion prunes too
        new, info = gsbp_amd.densify(params, st, dcfg, step, optimizer=opt, carry=dict(field=field),
                                     generator=torch.Generator(device=dev).manual_seed(77))
        results.append((new, info, opt, moments, field, st, params))
    new, info, opt, moments, field, st, old = results[0]
    # the counts are the reference plan's on the downloaded state
    th = dcfg.thresholds()
    want_kind, want_offsets = ref.plan(state.grad2d.cpu().numpy(), state.count.cpu().numpy(), old["scaling"].detach().cpu().numpy(),
                                       old["opacity"].detach().cpu().numpy(), th, True)
    counts = np.bincount(want_kind, minlength=4)
    assert [info["pruned"], info["kept"], info["cloned"], info["split"]] == counts.tolist() and min(counts) > 0
    n_out = info["n_after"]
    assert n_out == info["kept"] + 2 * (info["cloned"] + info["split"]) == int(want_offsets[-1]) and info["n_before"] == n
    assert np.array_equal(info["kind"].cpu().numpy(), want_kind)
    parent, child = info["parent"].long(), info["child"]
    for k in ("means", "scaling", "rotation", "opacity", "features_dc", "features_rest"):
        assert new[k].shape[0] == n_out and tuple(new[k].shape[1:]) == tuple(old[k].shape[1:])
    # the carried field and the gathered tensors are table[parent]; the Adam moments follow zero_new; step is kept
    assert torch.equal(info["carry"]["field"], field[parent])
    assert torch.equal(new["features_dc"].detach(), old["features_dc"].detach()[parent])
    k_of = info["kind"][parent]
    fresh = (k_of == 3) | ((k_of == 2) & (child == 1))
    assert int(fresh.sum()) > 0 and int((~fresh).sum()) > 0
    for key in ("means", "opacity", "features_dc"):
        assert opt.param_groups[["means", "scaling", "rotation", "opacity", "features_dc"].index(key)]["params"][0] is new[key]
        state_k = opt.state[new[key]]
        assert float(state_k["step"]) == 1.0
        for m in ("exp_avg", "exp_avg_sq"):
            want = moments[key][m][parent].clone()
            want[fresh] = 0
            assert torch.equal(state_k[m], want)
    assert len(opt.state) == 5 and all(p.shape[0] == n_out for g in opt.param_groups for p in g["params"])
    # the state is zeros of the new size, and the next step runs on the new set
    assert st.n == n_out and tuple(st.grad2d.shape) == (n_out,) and not st.grad2d.any() and not st.count.any()
    opt.zero_grad(set_to_none=True)
    image, meta = render_splats(new, vms[1], K, cfg.width, cfg.height, return_meta=True, means2d_grad=True)
    loss = gsbp_amd.photometric_loss(image, images[1])
    loss.backward()
    st.update(meta)
    opt.step()
    assert math.isfinite(float(loss.detach())) and all(bool(torch.isfinite(t).all()) for t in new.values())
    assert float(st.count.max()) == 1.0
    # a second call on the same inputs with the same generator seed: the same bits.  (The inputs are those of the loop's second pass,
    # whose round nobody has stepped since; the two passes themselves differ by the blend backward's atomics.)
    new2, info2 = results[1][0], results[1][1]
    again, info3 = gsbp_amd.densify({k: t.detach() for k, t in results[1][6].items()}, _state_copy(state, dev), dcfg,
                                    dcfg.reset_every + 100, carry=dict(field=field), generator=torch.Generator(device=dev).manual_seed(77))
    assert torch.equal(info3["parent"], info2["parent"]) and torch.equal(info3["child"], info2["child"])
    assert torch.equal(info3["carry"]["field"], info2["carry"]["field"])
    for k in ("means", "scaling", "rotation", "opacity", "features_dc"):
        assert torch.equal(again[k], new2[k].detach()), k
    other, _ = gsbp_amd.densify({k: t.detach() for k, t in results[1][6].items()}, _state_copy(state, dev), dcfg, dcfg.reset_every + 100,
                                generator=torch.Generator(device=dev).manual_seed(78))
    assert not torch.equal(other["means"], again["means"]) and torch.equal(other["scaling"], again["scaling"])  # the noise is the seed's
    # max_gaussians: nothing grows, the prune still runs
    capped, cinfo = gsbp_amd.densify({k: t.detach() for k, t in results[1][6].items()}, _state_copy(state, dev),
                                     gsbp_amd.DensifyConfig(grow_grad2d=grow, prune_opa=opa, grow_scale3d=0.06, prune_scale3d=0.25,
                                                            max_gaussians=n), dcfg.reset_every + 100)
    assert info2["n_after"] > n  # (the uncapped round grows the set)
    assert cinfo["cloned"] == cinfo["split"] == 0 and cinfo["n_after"] == cinfo["kept"] < n and cinfo["pruned"] >= info2["pruned"]


def _state_copy(state, dev):
    st = gsbp_amd.DensifyState(state.n, dev)
    st.grad2d, st.count = state.grad2d.clone(), state.count.clone()
    return st


def test_reset_opacity(dev):
    """opacity = min(opacity, logit(2 prune_opa)) in place, and that parameter's moments -- only that parameter's -- zeroed."""
    n = 300
    g = torch.Generator().manual_seed(1)
    splats = dict(means=torch.randn(n, 3, generator=g).to(dev).requires_grad_(True), opacity=(3.0 * torch.randn(n, generator=g)).to(dev).requires_grad_(True))
    opt = torch.optim.Adam([dict(params=[splats["means"]], lr=1e-3), dict(params=[splats["opacity"]], lr=1e-2)])
    (splats["means"].sum() + (splats["opacity"] ** 2).sum()).backward()
    opt.step()
    before = splats["opacity"].detach().clone()
    cfg = gsbp_amd.DensifyConfig(prune_opa=0.01)
    cap = math.log(0.02 / 0.98)
    assert gsbp_amd.reset_opacity(splats, opt, cfg) is splats
    assert torch.equal(splats["opacity"].detach(), before.clamp(max=cap)) and int((before > cap).sum()) > 100
    assert splats["opacity"].requires_grad and opt.param_groups[1]["params"][0] is splats["opacity"]
    assert not opt.state[splats["opacity"]]["exp_avg"].any() and not opt.state[splats["opacity"]]["exp_avg_sq"].any()
    assert opt.state[splats["means"]]["exp_avg"].any() and float(opt.state[splats["opacity"]]["step"]) == 1.0
