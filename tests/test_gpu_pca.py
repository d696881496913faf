"""fit_pca / pca_transform / pca_colors / render_pca on the GPU against the float64 reference and the bounds of tests/pca_ref.py.

Let u = 2^-24.  Every covariance entry lies within E_ab = 2 (N + 2) u sum_g |x_ga - mu_a||x_gb - mu_b| / (N - 1) of the float64
covariance; each of the top 3 components within the Davis-Kahan angle 2 ||E||_2 / gap_j of the float64 one, with the same sign; each
explained variance within ||E||_2 (Weyl).  test_pca_cpu.py asserts on the reference alone that every case's angle bound is at most
0.05 rad.  Each test prints what it measured before it asserts."""
import numpy as np
import pytest
import torch

import gsbp_amd
from gsbp_amd import pca
from gsbp_amd import synthetic as syn

import pca_ref

pytestmark = pytest.mark.gpu
U = pca_ref.U


def _check_fit(dev, X, what=""):
    """Fit X [N, D] (numpy fp32) on the device; covariance, components and variances against float64 within the bounds."""
    Xd = torch.from_numpy(X).to(dev)
    mean, cov = pca._covariance(Xd)
    E = pca_ref.cov_bound(X)
    err = np.abs(cov.cpu().numpy() - pca_ref.cov64(X))
    print(f"{what} N={X.shape[0]} D={X.shape[1]}: max cov error {err.max():.3e}, max error / bound {(err / E).max():.3e}")
    assert (err <= E).all()
    assert np.abs(mean.cpu().numpy().astype(np.float64) - pca_ref.mean64(X)).max() <= 2 * U * np.abs(X).max()
    basis = gsbp_amd.fit_pca(Xd, 3)
    theta, norm = pca_ref.angle_bounds(X, 3, E)
    assert (theta <= pca_ref.ANGLE_CAP).all()
    _, comps, var, ratio = pca_ref.fit(X, 3)
    got = basis.components.cpu().numpy().astype(np.float64)
    angles = [pca_ref.angle(comps[j], got[j]) for j in range(3)]
    print(f"   angles {angles} (bounds {theta}), variance errors {np.abs(basis.explained_variance.numpy() - var)} (bound {norm:.3e})")
    for j in range(3):
        assert angles[j] <= theta[j] and float(comps[j] @ got[j]) > 0.0
    assert (np.abs(basis.explained_variance.numpy() - var) <= norm).all()
    # (the ratio divides by the trace, whose error is at most trace(E))
    assert np.allclose(basis.explained_variance_ratio.numpy(), ratio, rtol=0, atol=(norm + np.trace(E)) / var.sum())
    assert basis.n_samples == X.shape[0] and basis.mean.dtype == torch.float32 and basis.components.shape == (3, X.shape[1])
    return basis


@pytest.mark.parametrize("case", range(len(pca_ref.FIT_CASES)))
def test_fit_against_float64(dev, case):
    """(N, D) = (20 000, 64), (50 000, 36), (4097, 512), (3001, 1028): all four run the covariance, angle and variance checks."""
    _check_fit(dev, pca_ref.make_case(*pca_ref.FIT_CASES[case]))


def _bits(basis):
    return [basis.mean.view(torch.int32), basis.components.view(torch.int32), basis.explained_variance]


@pytest.mark.parametrize("D", [1, 3, 30, 1024])
def test_edges_and_storage(dev, D):
    """N = 2, 63, 4097 x D = 1, 3, 30, 1024: the covariance within pca_ref.cov_bound_with_mean (two rows at a mean of 20 have columns
    whose spread is a few ulps of the mean, where the exact fp32 evaluation itself leaves cov_bound: see there); padded storage (NaN in the padding, which must never
    be read) and a column slice at an odd offset equal the contiguous result bit for bit, for the fit, the transform and colours."""
    k = min(3, D)
    for N in (2, 63, 4097):
        X = pca_ref.make_case(N, D, seed=1000 * D + N)
        Xd = torch.from_numpy(X).to(dev)
        mean, cov = pca._covariance(Xd)
        err = np.abs(cov.cpu().numpy() - pca_ref.cov64(X))
        assert (err <= pca_ref.cov_bound_with_mean(X)).all(), (N, D, err.max())
        b0 = gsbp_amd.fit_pca(Xd, k)
        y0 = gsbp_amd.pca_transform(Xd, b0)
        wide = torch.full((N, ((D + 3) // 4) * 4 + 8), float("nan"), device=dev)  # 16-B aligned rows, padded
        wide[:, :D] = Xd
        odd = torch.full((N, D + 7), float("nan"), device=dev)                     # 4-B aligned rows only
        odd[:, 5:5 + D] = Xd
        for view in (wide[:, :D], odd[:, 5:5 + D]):
            b = gsbp_amd.fit_pca(view, k)
            assert all(torch.equal(p, q) for p, q in zip(_bits(b), _bits(b0))), (N, D)
            assert torch.equal(gsbp_amd.pca_transform(view, b0).view(torch.int32), y0.view(torch.int32))
        assert wide[:, :D].data_ptr() == wide.data_ptr()
        assert bool(torch.isfinite(y0).all()) and y0.shape == (N, k)
        bound = pca_ref.transform_bound(X, b0.mean.cpu().numpy(), b0.components.cpu().numpy())
        y64 = pca_ref.transform64(X, b0.mean.cpu().numpy(), b0.components.cpu().numpy())
        assert (np.abs(y0.cpu().numpy() - y64) <= bound).all(), (N, D)
    # half inputs are widened like transfer's rows
    Xh = Xd.half()
    assert all(torch.equal(p, q) for p, q in zip(_bits(gsbp_amd.fit_pca(Xh, k)), _bits(gsbp_amd.fit_pca(Xh.float(), k))))


def test_determinism_and_row_order(dev):
    X = pca_ref.make_case(*pca_ref.FIT_CASES[0])
    Xd = torch.from_numpy(X).to(dev)
    a, b = gsbp_amd.fit_pca(Xd), gsbp_amd.fit_pca(Xd.clone())
    assert all(torch.equal(p, q) for p, q in zip(_bits(a), _bits(b)))
    c1, c2 = pca._covariance(Xd)[1], pca._covariance(Xd)[1]
    assert torch.equal(c1, c2)
    perm = np.random.default_rng(5).permutation(X.shape[0])
    _check_fit(dev, X[perm], "row-permuted")


def test_centring(dev):
    """A constant vector of 100 standard deviations per column on every row: the components stay within the angle bound of the
    float64 fit of the shifted rows.  An uncentred Gram (sum x x^T - N mu mu^T in fp32) loses every digit here."""
    X = pca_ref.shifted(pca_ref.make_case(*pca_ref.FIT_CASES[0]))
    X64 = X.astype(np.float64)
    assert (np.abs(X64.mean(axis=0)) > 99 * X64.std(axis=0)).all()
    _check_fit(dev, X, "shifted by 100 sigma")


def test_transform_and_colours(dev):
    X = pca_ref.make_case(*pca_ref.FIT_CASES[0])
    Xd = torch.from_numpy(X).to(dev)
    for k in (1, 3, 16):
        basis = gsbp_amd.fit_pca(Xd, k)
        Y = gsbp_amd.pca_transform(Xd, basis)
        mu, V = basis.mean.cpu().numpy(), basis.components.cpu().numpy()
        err = np.abs(Y.cpu().numpy() - pca_ref.transform64(X, mu, V))
        bound = pca_ref.transform_bound(X, mu, V)
        print(f"k={k}: max transform error {err.max():.3e}, max error / bound {(err / bound).max():.3e}")
        assert Y.shape == (X.shape[0], k) and (err <= bound).all()
    basis = gsbp_amd.fit_pca(Xd, 3)
    Y = gsbp_amd.pca_transform(Xd, basis)
    colors, lo, hi = gsbp_amd.pca_colors(Xd, basis)
    assert lo.view(torch.int32).item() == Y.min().view(torch.int32).item()
    assert hi.view(torch.int32).item() == Y.max().view(torch.int32).item()
    assert colors.shape == (X.shape[0], 3) and float(colors.min()) >= 0.0 and float(colors.max()) <= 1.0
    want = (Y - lo) / (hi - lo)
    ulp = np.spacing(np.maximum(np.abs(want.cpu().numpy()), np.float32(2.0 ** -126)).astype(np.float32))
    assert (np.abs(colors.cpu().numpy().astype(np.float64) - want.cpu().numpy()) <= 2 * ulp).all()
    # basis=None fits PCA(3) itself
    c2, lo2, hi2 = gsbp_amd.pca_colors(Xd)
    assert torch.equal(c2, colors) and torch.equal(lo2, lo) and torch.equal(hi2, hi)
    # one lo / hi for all channels, as the reference's np.min(..., axis=(0, 1)): against the float64 colours of the product's Y
    ref, _, _ = pca_ref.colors64(Y.cpu().numpy().astype(np.float64))
    assert np.abs(colors.cpu().numpy() - ref).max() <= 4 * U


def test_zero_variance_field(dev):
    """All rows equal.  The choice: the mean is the row exactly, the covariance exactly 0, the components the unit vectors eigh
    returns for a zero matrix (finite), explained variance and ratio 0, and the colours 0.5 everywhere (hi == lo)."""
    row = torch.randn(48, generator=torch.Generator().manual_seed(0))
    Xd = row.repeat(1000, 1).to(dev)
    basis = gsbp_amd.fit_pca(Xd)
    assert torch.equal(basis.mean.cpu(), row)
    assert bool(torch.isfinite(basis.components).all())
    assert torch.allclose(basis.components.norm(dim=1).cpu(), torch.ones(3))
    assert float(basis.explained_variance.abs().max()) == 0.0 and float(basis.explained_variance_ratio.abs().max()) == 0.0
    colors, lo, hi = gsbp_amd.pca_colors(Xd, basis)
    assert float(lo) == 0.0 and float(hi) == 0.0 and bool((colors == 0.5).all())


def test_nan_row_raises(dev):
    Xd = torch.from_numpy(pca_ref.make_case(5000, 40, seed=9)).to(dev)
    Xd[1234, 7] = float("nan")
    with pytest.raises(gsbp_amd.GwbpError, match="NaN"):
        gsbp_amd.fit_pca(Xd)
    Xd[1234, 7] = float("inf")
    with pytest.raises(gsbp_amd.GwbpError, match="NaN or infinite"):
        gsbp_amd.fit_pca(Xd)


def _scene(cfg, dev):
    means, quats, scales, opac = (t.to(dev) for t in syn.activate(syn.make_scene(cfg)))
    return means, quats, scales, opac, syn.make_cameras(cfg).to(dev), syn.intrinsics(cfg).to(dev)


def _field(cfg, dev, scene):
    means, quats, scales, opac, vms, K = scene
    return gsbp_amd.create_feature_field(means, quats, scales, opac, vms, K, cfg.width, cfg.height,
                                         lambda v: syn.make_feature_map(cfg, v, device=dev), cfg.feat_dim)


@pytest.mark.parametrize("kw", [{}, {"camera_model": "fisheye", "rasterize_mode": "antialiased"}])
def test_render_gaussians_mode(dev, kw):
    cfg = syn.CONFIGS["T1"]
    scene = _scene(cfg, dev)
    means, quats, scales, opac, vms, K = scene
    field = _field(cfg, dev, scene)
    frames = list(gsbp_amd.render_pca(means, quats, scales, opac, field, vms, K, cfg.width, cfg.height, mode="gaussians",
                                      scale=0.2, **kw))
    colors, _, _ = gsbp_amd.pca_colors(field)
    assert len(frames) == cfg.n_views
    for v, frame in enumerate(frames):
        out, _, _ = gsbp_amd.rasterization(means, quats, scales * 0.2, opac, colors, vms[v:v + 1], K[None], cfg.width, cfg.height,
                                           **kw)
        want = (out[0].clamp(0.0, 1.0) * 255.0).to(torch.uint8)
        assert frame.dtype == torch.uint8 and frame.shape == (cfg.height, cfg.width, 3) and torch.equal(frame, want)
        assert int(frame.max()) > 0


def test_render_renderings_mode(dev):
    """C1 (D = 32, where the literal wide render exists): render(F V^T) - mu V^T against rasterization(F) followed by a float64
    (x - mu) V^T on the host, per pixel within 2 (n_max + D + 4) u S, n_max the longest tile list and S = max_g sum_c |F_gc||V_jc| +
    |mu . V_j| (the weights of a pixel sum to at most 1).  The uint8 frames differ by at most one level, and only at pixels whose
    reference value lies within that bound of a level boundary."""
    cfg = syn.CONFIGS["C1"]
    scene = _scene(cfg, dev)
    means, quats, scales, opac, vms, K = scene
    field = _field(cfg, dev, scene)
    D = field.shape[1]
    basis, lo, hi, floats = pca._pca_frames(means, quats, scales, opac, field, vms, K, cfg.width, cfg.height, "renderings", None,
                                            1.0, {})
    floats = [f.clone() for f in floats]
    frames = list(gsbp_amd.render_pca(means, quats, scales, opac, field, vms, K, cfg.width, cfg.height, mode="renderings",
                                      basis=basis))
    mu, V = basis.mean.cpu().numpy().astype(np.float64), basis.components.cpu().numpy().astype(np.float64)
    S = (np.abs(field.cpu().numpy().astype(np.float64)) @ np.abs(V).T).max(axis=0) + np.abs(V @ mu)  # [3]
    lo64, hi64 = float(lo), float(hi)
    for v in range(cfg.n_views):
        wide, _, meta = gsbp_amd.rasterization(means, quats, scales, opac, field, vms[v:v + 1], K[None], cfg.width, cfg.height)
        offs = meta["isect_offsets"].reshape(-1).cpu().numpy().astype(np.int64)
        n_max = int(np.diff(np.append(offs, meta["flatten_ids"].shape[0])).max())
        ref = (wide[0].cpu().numpy().astype(np.float64) - mu) @ V.T
        bound = 2.0 * (n_max + D + 4) * U * S
        err = np.abs(floats[v].cpu().numpy() - ref)
        print(f"view {v}: n_max {n_max}, max error {err.max(axis=(0, 1))}, bound {bound}")
        assert (err <= bound).all()
        t = (ref - lo64) / (hi64 - lo64) * 255.0
        want = np.clip(t, 0.0, 255.0).astype(np.uint8)
        got = frames[v].cpu().numpy()
        diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
        assert diff.max() <= 1
        slack = bound * 255.0 / (hi64 - lo64) + 8 * 256 * U  # the bound in levels + the fp32 normalisation's own rounding
        assert (np.abs(t - np.rint(t))[diff > 0] <= np.broadcast_to(slack, t.shape)[diff > 0]).all()
        assert got.max() > got.min()


def test_c2_frame_needs_no_wide_image(dev):
    """One C2-geometry frame (1 M Gaussians, D = 512, 1600 x 1060) per mode, the fit included: the peak memory above the scene, the
    field and the rasterizer's workspace stays below ONE [H, W, 16] render -- no [H, W, D] image (3.5 GB), no second [N, D]."""
    cfg = syn.CONFIGS["C2"]
    means, quats, scales, opac, vms, K = _scene(cfg, dev)
    g = torch.Generator(device=dev).manual_seed(0)
    field = torch.randn(cfg.n_gaussians, cfg.feat_dim, device=dev, generator=g)
    field += 3.0 * torch.randn(cfg.feat_dim, device=dev, generator=g)  # a common component, as lifted features have
    field /= field.norm(dim=1, keepdim=True)
    W, H = cfg.width, cfg.height
    gsbp_amd.rasterization(means, quats, scales, opac, field[:, :3].contiguous(), vms[:1], K[None], W, H, want_meta=False)  # workspace
    torch.cuda.synchronize()
    for mode, scale in (("gaussians", 0.2), ("renderings", 1.0)):
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        frame = next(gsbp_amd.render_pca(means, quats, scales, opac, field, vms[:1], K, W, H, mode=mode, scale=scale))
        torch.cuda.synchronize()
        extra = torch.cuda.max_memory_allocated(dev) - base
        print(f"{mode}: peak extra memory {extra / 2 ** 20:.1f} MiB (one [H, W, 16] render: {H * W * 16 * 4 / 2 ** 20:.1f} MiB)")
        assert frame.shape == (H, W, 3) and frame.dtype == torch.uint8 and int(frame.max()) > int(frame.min())
        assert extra < H * W * 16 * 4
