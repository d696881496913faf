"""train_scene with the feature term: the reference trainer's two-render step on the HIP path.  The targets are a hidden latent field
[512, 16] and decoder [16, 32] rendered on T0's true scene; the start is every second Gaussian of it, zero latents and a seeded
torch.rand decoder.

    * 60 steps with densify rounds inside: `features` follows every round, the feature loss of the last pass over the views is below
      the first pass's
    * the feature term reaches the geometry: means.grad of one step differs from the step without it and is the sum of the two terms'
      own gradients
    * the decoder is not a per-Gaussian table, even when latent_dim == N
    * an MCMC run keeps the shapes together; feature_fn=None returns the history it always did; one run through the command line
"""
import functools
import json
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gsbp_amd  # noqa: E402
import raster_grad_ref as rg  # noqa: E402
import run_train  # noqa: E402
from gsbp_amd.polish import render_splats, splat_geometry  # noqa: E402
from test_gpu_densify import probe_thresholds, t0_training_setup  # noqa: E402

pytestmark = pytest.mark.gpu
LATENT, FEATURE = 16, 32


@functools.lru_cache(maxsize=None)
def setup(dev):
    """T0's training setup and the views' feature maps; computed once, never modified."""
    cfg, start, K, vms, images = t0_training_setup(dev)
    full = {k: t.to(dev) for k, t in gsbp_amd.synthetic.make_scene(cfg).items()}
    gen = torch.Generator().manual_seed(77)
    latents = torch.rand(full["means"].shape[0], LATENT, generator=gen).to(dev)
    decoder = (torch.rand(LATENT, FEATURE, generator=gen) / LATENT).to(dev)
    with torch.no_grad():
        maps = [gsbp_amd.render_latents(*splat_geometry(full), latents, vms[v], K, cfg.width, cfg.height)[0] @ decoder
                for v in range(vms.shape[0])]
    assert float(maps[0].abs().max()) > 0.05
    return dict(cfg=cfg, start=start, K=K, vms=vms, images=images, maps=maps)


def train(s, steps, start=None, **kw):
    cfg = s["cfg"]
    kw.setdefault("feature_fn", lambda v: s["maps"][v])
    kw.setdefault("feature_dim", FEATURE)
    kw.setdefault("latent_dim", LATENT)
    return gsbp_amd.train_scene(s["start"] if start is None else start, s["vms"], s["K"], cfg.width, cfg.height, lambda v: s["images"][v],
                                steps, seed=3, **kw)


def test_sixty_steps_with_rounds_inside(dev):
    s = setup(dev)
    _, _, grow, opa = probe_thresholds(dev, s["start"], s["K"], s["vms"], s["images"], s["cfg"])
    dcfg = gsbp_amd.DensifyConfig(grow_grad2d=grow, prune_opa=opa, grow_scale3d=10.0, prune_scale3d=100.0, refine_start_iter=10,
                                  refine_every=10)
    trained, hist = train(s, 60, cfg=dcfg)
    sizes, rounds, floss = hist["n"], hist["rounds"], hist["feature_loss"]
    assert [r["step"] for r in rounds] == [20, 30, 40, 50] and len(set(sizes)) > 1
    for r in rounds:  # the step behind a round rendered `features` with the round's N' rows (render_latents refuses another count)
        assert sizes[r["step"] + 1] == r["n_after"]
    n = rounds[-1]["n_after"]
    assert tuple(trained["features"].shape) == (n, LATENT) and tuple(trained["means"].shape) == (n, 3)
    assert tuple(hist["decoder"].shape) == (LATENT, FEATURE) and bool(torch.isfinite(hist["decoder"]).all())
    assert bool(torch.isfinite(trained["features"]).all()) and float(trained["features"].abs().max()) > 0
    assert len(floss) == len(hist["loss"]) == 60 and all(math.isfinite(v) for v in floss)
    V = s["vms"].shape[0]
    first, last = sum(floss[:V]) / V, sum(floss[-V:]) / V
    print(f"feature loss, mean over a pass of {V} views: first {first:.5f}, last {last:.5f}, ratio {last / first:.3f}; N {sizes[0]} -> {n}")
    assert last / first < 1.0


def _crop(s, w=32, h=16):
    """The w x h pixels at the centre of view 0: (K, image, map).  Two tiles: a Gaussian's blend gradient is then the sum of at most two
    partial sums onto zero, in either order the same bits (tests/test_gpu_mcmc.py::test_the_default_path_is_unchanged), so what differs
    between two evaluations is arithmetic, not the order of the atomics."""
    cfg = s["cfg"]
    x0, y0 = (cfg.width - w) // 2, (cfg.height - h) // 2
    K = s["K"].clone()
    K[0, 2] -= x0
    K[1, 2] -= y0
    return K, s["images"][0][y0:y0 + h, x0:x0 + w].contiguous(), s["maps"][0][y0:y0 + h, x0:x0 + w].contiguous(), w, h


def _step_gradients(dev, s, latents, decoder, weight_photo, weight_feature):
    K, image_t, map_t, w, h = _crop(s)
    work = {k: t.clone().requires_grad_(True) for k, t in s["start"].items()}
    geometry = splat_geometry(work)
    loss = 0.0
    if weight_photo:
        image = render_splats(work, s["vms"][0], K, w, h, geometry=geometry)
        loss = loss + weight_photo * gsbp_amd.photometric_loss(image, image_t)
    if weight_feature:
        out, _ = gsbp_amd.render_latents(*geometry, latents, s["vms"][0], K, w, h)
        loss = loss + weight_feature * gsbp_amd.decoded_loss(out, decoder, map_t)
    loss.backward()
    return {k: work[k].grad.detach().cpu() for k in ("means", "scaling", "rotation", "opacity")}


SUM_FACTOR = 4.0  # tests/test_gpu_raster_grad.py's; measured ratios beside the assertion below


def test_the_feature_term_reaches_the_geometry_and_adds_to_the_photometric_one(dev):
    """The floor rule.  Truth: the two terms' own float32 gradients, widened and added in float64.  Floor: the same two added in float32
    -- what one rounding per entry costs.  Kernel path: the gradient of the step with both terms, whose two backwards meet at the leaves
    (and, for scaling and opacity, in front of one exp / sigmoid backward instead of behind two).  kernel <= SUM_FACTOR x floor per
    tensor and figure.  A dropped or doubled term is off by 0.1 .. 1 against floors near 3e-8.
    Measured on an MI355X, kernel / floor (Frobenius, max-abs): means 1.00, 1.00 (the same bits as the float32 sum), scaling 1.31, 1.00,
    rotation 1.00, 1.00, opacity 1.32, 1.00; floors 2.5e-8 .. 2.9e-8 and 3.0e-8 .. 4.0e-8."""
    s = setup(dev)
    n = s["start"]["means"].shape[0]
    gen = torch.Generator().manual_seed(5)
    latents, decoder = torch.rand(n, LATENT, generator=gen).to(dev), torch.rand(LATENT, FEATURE, generator=gen).to(dev)
    both = _step_gradients(dev, s, latents, decoder, 1.0, 1.0)
    photo = _step_gradients(dev, s, latents, decoder, 1.0, 0.0)
    feat = _step_gradients(dev, s, latents, decoder, 0.0, 1.0)
    for k in both:
        truth = photo[k].double() + feat[k].double()
        floor, kernel = rg.errors(photo[k] + feat[k], truth), rg.errors(both[k], truth)
        away, _ = rg.errors(both[k], photo[k].double())
        print(f"{k:9s} floor {floor[0]:.2e} / {floor[1]:.2e}   both terms {kernel[0]:.2e} / {kernel[1]:.2e}   ratio "
              f"{kernel[0] / max(floor[0], 1e-300):.2f} / {kernel[1] / max(floor[1], 1e-300):.2f}   against photo alone: {away:.2e}")
        assert float(feat[k].abs().max()) > 0 and away > 1e-2, k
        assert floor[0] > 0 and floor[1] > 0, k
        assert kernel[0] <= SUM_FACTOR * floor[0] and kernel[1] <= SUM_FACTOR * floor[1], (k, floor, kernel)
    # ... and through train_scene: one step from the caller's latents moves the means differently with and without the term
    start = dict(s["start"], features=latents)
    with_term = train(s, 1, start=start, decoder=decoder)[0]["means"]
    without = train(s, 1, start=start, decoder=decoder, feature_weight=0.0)[0]["means"]
    assert not torch.equal(with_term, without)


def test_a_decoder_of_n_rows_is_not_relocated(dev):
    """16 Gaussians, latent_dim 16: a round moves every float32 tensor of the dict with N rows; the decoder has N rows and is not one."""
    s = setup(dev)
    start = {k: t[::16].contiguous() for k, t in s["start"].items()}
    assert start["means"].shape[0] == LATENT
    gen = torch.Generator().manual_seed(9)
    d0 = torch.rand(LATENT, FEATURE, generator=gen).to(dev)
    start["features"] = torch.rand(LATENT, LATENT, generator=gen).to(dev)
    one = train(s, 1, start=start, decoder=d0)[1]["decoder"]
    step = (one - d0).abs()
    assert 0 < float(step.max()) <= 2.5e-3 * (1 + 1e-3)  # the first Adam step moves an entry by lr at most
    grows = gsbp_amd.DensifyConfig(grow_grad2d=0.0, grow_scale3d=10.0, prune_scale3d=100.0, refine_start_iter=0, refine_every=1)
    never = gsbp_amd.DensifyConfig(refine_start_iter=1000)
    trained, hist = train(s, 2, start=start, decoder=d0, cfg=grows)
    plain = train(s, 2, start=start, decoder=d0, cfg=never)[1]["decoder"]
    assert [r["step"] for r in hist["rounds"]] == [1] and hist["rounds"][0]["n_after"] != LATENT
    n = hist["rounds"][0]["n_after"]
    assert tuple(trained["features"].shape) == (n, LATENT) and tuple(trained["means"].shape) == (n, 3)
    assert tuple(hist["decoder"].shape) == (LATENT, FEATURE)
    # two Adam steps either way (the round comes behind the second): the same table up to the float atomics of step 1's gradients
    assert float((hist["decoder"] - plain).abs().mean()) < 1e-4 and float((hist["decoder"] - d0).abs().max()) <= 2 * 2.5e-3 * (1 + 1e-3)


def test_mcmc_keeps_the_shapes_together(dev):
    s = setup(dev)
    cap = 290
    trained, hist = train(s, 30, strategy=gsbp_amd.MCMCConfig(refine_start_iter=5, refine_every=10, cap_max=cap), opacity_reg=0.01,
                          scale_reg=0.01)
    assert [r["step"] for r in hist["rounds"]] == [10, 20] and hist["rounds"][-1]["n_after"] == trained["means"].shape[0] > 256
    n = trained["means"].shape[0]
    assert tuple(trained["features"].shape) == (n, LATENT) and tuple(hist["decoder"].shape) == (LATENT, FEATURE)
    assert all(math.isfinite(v) for v in hist["loss"] + hist["feature_loss"]) and bool(torch.isfinite(trained["features"]).all())


def test_without_feature_fn_the_history_is_the_old_one(dev):
    s = setup(dev)
    trained, hist = train(s, 3, feature_fn=None, feature_dim=None)
    assert set(hist) == {"loss", "n", "rounds", "resets", "carry", "sh_degree"} and "features" not in trained
    with pytest.raises(gsbp_amd.GwbpError, match="feature_dim"):
        train(s, 1, feature_dim=None)


def test_run_train_with_a_feature_field(tmp_path, dev):
    out = str(tmp_path / "train")
    rc = run_train.main(["--synthetic", "T0", "--feature-dim", str(FEATURE), "--latent-dim", str(LATENT), "--steps", "20", "--seed", "3",
                         "--out", out])
    assert rc == 0
    with open(os.path.join(out, "history.json")) as f:
        hist = json.load(f)
    assert len(hist["feature_loss"]) == len(hist["loss"]) == 20 and all(math.isfinite(v) for v in hist["feature_loss"])
    assert (hist["feature_dim"], hist["latent_dim"], hist["feature_weight"]) == (FEATURE, LATENT, 1.0)
    saved = torch.load(os.path.join(out, "features.pt"))
    n = hist["n"][-1]
    assert tuple(saved["features"].shape) == (n, LATENT) and tuple(saved["decoder"].shape) == (LATENT, FEATURE)
    assert tuple(torch.load(os.path.join(out, "trained.pt"))["features"].shape) == (n, LATENT)
