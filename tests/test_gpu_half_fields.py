"""fp16 / bf16 finished fields on the GPU.  The contract: a half field gives the BITS the fp32 kernel gives on field.float(), and no
fp32 copy of the field is allocated; a typed finalise equals the fp32 finalise rounded once by torch's .to(dtype).

Shapes: N = 300 (no multiple of any block's rows), D in {1, 6, 64, 260, 516} (one element, no multiple of 4, aligned, and two chunks of
regions.hip's 256 columns with a remainder), three layouts (contiguous; row stride D + 4: the 8-B vector path where D % 4 == 0; row
stride D + 1 on a view that starts one element into its buffer: 2-B element loads), padding filled with NaN so that a read beyond D
shows."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gsbp_amd
from gsbp_amd import pca, sample, spatial, synthetic as syn

import half_fields_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF = (torch.float16, torch.bfloat16)
N, DIMS, LAYOUTS = 300, (1, 6, 64, 260, 516), ("contiguous", "stride D + 4", "stride D + 1, offset 1")
P, N_POS, M_SRC, K_NN, K_MEANS, K_PCA = 3, 2, 40, 5, 7, 3


def _field32(n: int, d: int, dtype, seed: int) -> torch.Tensor:
    """Values drawn in fp32 and rounded to dtype (returned widened again, on the host), with the special rows."""
    g = torch.Generator().manual_seed(seed)
    f = torch.randn(n, d, generator=g)
    f[0] = 0.0
    f[1] = float("nan")
    f[2] = float("inf")
    if dtype == torch.float16:
        f[3, 0::2], f[3, 1::2] = 65504.0, -65504.0
        f[4] = 2.0 ** -24  # the smallest fp16 subnormal
    else:
        f[3, 0::2], f[3, 1::2] = 3e38, -3e38
        f[4] = 2.0 ** -130  # a bfloat16 subnormal
    h = f.to(dtype)
    assert bool((h[4].float() > 0).all()) and bool(torch.isfinite(h[3].float()).all())
    return h.float()


def _layout(values32: torch.Tensor, dtype, layout: str, dev) -> torch.Tensor:
    n, d = values32.shape
    if layout == "contiguous":
        return values32.to(dtype).to(dev)
    if layout == "stride D + 4":
        buf = torch.full((n, d + 4), float("nan"), dtype=dtype, device=dev)
        view = buf[:, :d]
    else:
        buf = torch.full((n * (d + 1) + 1,), float("nan"), dtype=dtype, device=dev)
        view = buf[1:].view(n, d + 1)[:, :d]
        assert view.data_ptr() % 4 == 2  # 2-B aligned only
    view.copy_(values32.to(dtype))
    return view


@functools.lru_cache(maxsize=None)
def _operands(d: int, n: int = N):
    """The small fp32 operands of every consumer, on the host: made once per D, never modified."""
    g = torch.Generator().manual_seed(77 + d)
    idx = torch.randint(0, n, (n, K_NN), generator=g, dtype=torch.int32)
    idx[torch.rand(n, K_NN, generator=g) < 0.15] = -1
    idx[7] = -1  # a row without a neighbour
    w = torch.rand(n, K_NN, generator=g)
    w[torch.rand(n, K_NN, generator=g) < 0.1] = 0.0
    return dict(prompts=torch.randn(P, d, generator=g), sources=torch.randn(M_SRC, d, generator=g),
                centroids=torch.randn(K_MEANS, d, generator=g), labels=torch.randint(-1, K_MEANS, (n,), generator=g),
                weights=torch.rand(n, generator=g), idx=idx, w=w, mean=torch.randn(d, generator=g) * 0.1,
                comps=torch.randn(min(K_PCA, d), d, generator=g))


def _consumers(op, dev):
    o = {k: v.to(dev) for k, v in op.items()}
    basis = pca.PCABasis(o["mean"], o["comps"], None, None, 0)
    return {
        "prompt_scores": lambda f: (gsbp_amd.prompt_scores(f, o["prompts"]), gsbp_amd.prompt_mask(f, o["prompts"], N_POS)),
        "knn_search": lambda f: gsbp_amd.knn_search(f, o["sources"], K_NN),
        "kmeans_assign": lambda f: gsbp_amd.kmeans_assign(f, o["centroids"], "euclidean"),  # (euclidean: with the bias)
        "cluster_sums": lambda f: gsbp_amd.cluster_sums(f, o["labels"], K_MEANS, o["weights"]),
        "neighbor_similarity": lambda f: gsbp_amd.neighbor_similarity(f, o["idx"]),
        "neighbor_mean": lambda f: (spatial.neighbor_mean(f, o["idx"]),),
        "neighbor_blend": lambda f: sample.neighbor_blend(f, o["idx"], o["w"]),
        "column_means": lambda f: (pca._covariance(f)[0],),
        "centered_gram": lambda f: (pca._covariance(f)[1],),
        "pca_project": lambda f: (gsbp_amd.pca_transform(f, basis),),
    }


CONSUMERS = ("prompt_scores", "knn_search", "kmeans_assign", "cluster_sums", "neighbor_similarity", "neighbor_mean",
             "neighbor_blend", "column_means", "centered_gram", "pca_project")


def _bits(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def _same(a, b) -> bool:
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(_bits(x), _bits(y))
                                    for x, y in zip(a, b))


@pytest.mark.parametrize("dtype", HALF, ids=["fp16", "bf16"])
@pytest.mark.parametrize("name", CONSUMERS)
def test_half_field_gives_the_bits_of_the_widened_field(dev, name, dtype):
    for d in DIMS:
        call = _consumers(_operands(d), dev)[name]
        values = _field32(N, d, dtype, seed=d)
        want = call(values.to(dev))  # the same Python function on field.float()
        assert all(t.dtype != dtype for t in want)  # results keep their dtypes: nothing comes out in half
        for layout in LAYOUTS:
            f = _layout(values, dtype, layout, dev)
            assert f.dtype == dtype and torch.equal(_bits(f.float()), _bits(values))
            got = call(f)
            assert _same(got, want), (name, d, layout)
            assert _same(call(f), got), (name, d, layout, "second run")


@pytest.mark.parametrize("dtype", HALF, ids=["fp16", "bf16"])
@pytest.mark.parametrize("name", CONSUMERS)
def test_half_field_is_read_without_a_second_field(dev, name, dtype):
    """The peak of the allocator over the call on a half field is at most the peak over the same call on an fp32 field made beforehand:
    everything else the two calls allocate is the same, and a .float() copy of the field would add exactly 4 N D bytes."""
    n, d = 4096, 512
    call = _consumers(_operands(d, n), dev)[name]
    g = torch.Generator().manual_seed(5)
    f32 = torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=1).to(dtype).float().to(dev)
    f16 = f32.to(dtype)
    peaks = []
    for f in (f32, f16):
        call(f)  # (warm: the library, the allocator's pools)
        torch.cuda.synchronize(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        call(f)
        torch.cuda.synchronize(dev)
        peaks.append(torch.cuda.max_memory_allocated(dev))
    print(f"{name} {dtype}: peak {peaks[0]} B on fp32, {peaks[1]} B on half, a copy would add {4 * n * d} B")
    assert peaks[1] <= peaks[0], (name, peaks, 4 * n * d)


@pytest.mark.parametrize("dtype", HALF, ids=["fp16", "bf16"])
def test_fits_and_smoothing_take_a_half_field(dev, dtype):
    """What sits on the ten kernels: fit_pca and smooth_features are bit-equal to their result on field.float() (every [N, D] pass is);
    fit_kmeans runs its Lloyd loop on the half field and returns float32 centroids whose assignment is its labels."""
    g = torch.Generator().manual_seed(11)
    n, d = 700, 36
    centres = torch.randn(5, d, generator=g)
    f32 = torch.nn.functional.normalize(centres[torch.randint(0, 5, (n,), generator=g)] + 0.1 * torch.randn(n, d, generator=g), dim=1)
    f = f32.to(dtype).to(dev)
    a, b = gsbp_amd.fit_pca(f, 3), gsbp_amd.fit_pca(f.float(), 3)
    assert torch.equal(_bits(a.mean), _bits(b.mean)) and torch.equal(_bits(a.components), _bits(b.components))
    assert torch.equal(a.explained_variance, b.explained_variance)
    ca, cb = gsbp_amd.pca_colors(f, a), gsbp_amd.pca_colors(f.float(), b)
    assert _same(ca, cb)
    means = torch.rand(n, 3, generator=g).to(dev)
    sm, sm32 = gsbp_amd.smooth_features(means, f, k=6), gsbp_amd.smooth_features(means, f.float(), k=6)
    assert sm.dtype == torch.float32 and _same((sm,), (sm32,))
    km = gsbp_amd.fit_kmeans(f, 5, metric="cosine", iters=10, seed=3)
    assert km.centroids.dtype == torch.float32 and km.centroids.shape == (5, d) and km.labels.shape == (n,)
    assert int(km.counts.sum()) == n and int((km.counts > 0).sum()) == 5
    if km.reseeds == 0:  # (the empty-cluster rule moves rows by hand)
        assert torch.equal(gsbp_amd.kmeans_assign(f, km.centroids, "cosine")[0], km.labels)
    km_e = gsbp_amd.fit_kmeans(f, 5, metric="euclidean", iters=5, seed=3, init="sample")
    if km_e.reseeds == 0:
        assert torch.equal(gsbp_amd.kmeans_assign(f, km_e.centroids, "euclidean")[0], km_e.labels)
    protos, counts = gsbp_amd.class_prototypes(f, km.labels, 5)
    p32, c32 = gsbp_amd.class_prototypes(f.float(), km.labels, 5)
    assert _same((protos, counts), (p32, c32))


def _accumulators(n: int, d: int, ties, dev):
    g = torch.Generator().manual_seed(99 + d)
    F = torch.randn(n, d, generator=g)
    dd = torch.rand(n, generator=g) + 0.5
    F[:, 1::3] *= 1e-6
    F[:, 2::5] *= 1e-9
    dd[0] = 0.0
    F[1] = 0.0
    F[2], dd[2] = 0.0, 0.0
    if d >= 5:
        for i, m in enumerate(ties):
            F[3 + 2 * i] = torch.from_numpy(ref.tie_row(m, d))
            F[4 + 2 * i] = -F[3 + 2 * i]
            dd[3 + 2 * i] = dd[4 + 2 * i] = 1.0
    return F.to(dev), dd.to(dev)


@pytest.mark.parametrize("d", [1, 6, 64, 516])
@pytest.mark.parametrize("dtype,bits,ties", [(torch.float16, ref.f32_to_f16_bits, ref.F16_TIES),
                                             (torch.bfloat16, ref.f32_to_bf16_bits, ref.BF16_TIES)], ids=["fp16", "bf16"])
def test_typed_finalize_is_the_fp32_finalize_rounded_once(dev, dtype, bits, ties, d):
    eng = gsbp_amd.Engine(N, 64, 64, device=dev)
    F, dd = _accumulators(N, d, ties, dev)
    full = eng.finalize(F, dd).cpu()
    assert not bool(torch.isnan(full).any())
    half = eng.finalize_typed(F, dd, dtype)
    assert half.dtype == dtype and half.shape == F.shape
    got = half.cpu().view(torch.int16)
    assert torch.equal(got, full.to(dtype).view(torch.int16))
    assert np.array_equal(got.numpy().view(np.uint16), bits(full.numpy()))
    if d >= 5:
        for i, m in enumerate(ties):
            assert np.array_equal(full[3 + 2 * i].numpy(), ref.tie_row(m, d))  # the exact tie reached the rounding
    assert torch.equal(eng.finalize_typed(F, dd, torch.float32).cpu(), full)
    out = torch.empty(N, d, dtype=dtype, device=dev)
    assert eng.finalize_typed(F, dd, dtype, out=out) is out and torch.equal(out.cpu().view(torch.int16), got)
    with pytest.raises(gsbp_amd.GwbpError):
        eng.finalize_typed(F, dd, dtype, out=torch.empty(N, d, device=dev))
    with pytest.raises(gsbp_amd.GwbpError):
        eng.finalize_typed(F, dd, torch.float64)


def _t0(dev):
    cfg = syn.CONFIGS["T0"]
    gauss = [t.to(dev) for t in syn.activate(syn.make_scene(cfg))]
    return cfg, gauss, syn.make_cameras(cfg).to(dev), syn.intrinsics(cfg).to(dev)


@pytest.mark.parametrize("dtype", HALF, ids=["fp16", "bf16"])
def test_create_feature_field_returns_the_field_in_out_dtype(dev, dtype):
    cfg, gauss, vms, K = _t0(dev)
    maps = [syn.make_feature_map(cfg, v, device=dev) for v in range(cfg.n_views)]
    args = (*gauss, vms, K, cfg.width, cfg.height, lambda v: maps[v], cfg.feat_dim)
    field, F_rows, d, st = gsbp_amd.create_feature_field(*args, out_dtype=dtype, return_partials=True)
    assert st["overflow"] == 0 and field.dtype == dtype and field.shape == (cfg.n_gaussians, cfg.feat_dim)
    assert F_rows.dtype == torch.float32 and d.dtype == torch.float32 and float(field.float().abs().max()) > 0
    eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev)
    want = eng.finalize(F_rows, d)  # (of THIS run's accumulators: the order of their atomic sums does not enter)
    assert torch.equal(field.cpu().view(torch.int16), want.cpu().to(dtype).view(torch.int16))
    base, F0, d0, _ = gsbp_amd.create_feature_field(*args, return_partials=True)  # the default: what it returned before
    assert base.dtype == torch.float32 and torch.equal(_bits(base), _bits(eng.finalize(F0, d0)))
    with pytest.raises(ValueError):
        gsbp_amd.create_feature_field(*args, out_dtype=torch.float64)


@pytest.mark.parametrize("dtype", HALF, ids=["fp16", "bf16"])
def test_create_mask_feature_field_returns_the_field_in_out_dtype(dev, dtype):
    cfg, gauss, vms, K = _t0(dev)
    pairs = [syn.make_mask_features(cfg, v, 5, 8, device=dev) for v in range(cfg.n_views)]
    field, F_rows, d, st = gsbp_amd.create_mask_feature_field(*gauss, vms, K, cfg.width, cfg.height, lambda v: pairs[v], 8,
                                                              out_dtype=dtype, return_partials=True)
    assert st["overflow"] == 0 and field.dtype == dtype
    eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev)
    assert torch.equal(field.cpu().view(torch.int16), eng.finalize(F_rows, d).cpu().to(dtype).view(torch.int16))


def test_cli_writes_a_bf16_field_and_the_tools_read_it(tmp_path, dev):
    def run(script, *argv):
        r = subprocess.run([sys.executable, os.path.join(ROOT, script), *argv], capture_output=True, text=True)
        assert r.returncode == 0, (script, r.stderr[-2000:])

    out = str(tmp_path / "field")
    run("run_backproject.py", "--synthetic", "C1", "--field-dtype", "bf16", "--no-prune", "--results-dir", out)
    path = os.path.join(out, "features_lseg.pt")
    field = torch.load(path)
    cfg = syn.CONFIGS["C1"]
    assert field.dtype == torch.bfloat16 and field.shape == (cfg.n_gaussians, cfg.feat_dim)
    norms = field.float().norm(dim=1)
    assert float(norms.max()) < 1.01 and float(norms[norms > 0].min()) > 0.99
    seg_out, pca_out = str(tmp_path / "segment"), str(tmp_path / "pca")
    run("run_segment.py", "--synthetic", "C1", "--features", path, "--max-views", "1", "--out", seg_out)
    mask3d = torch.load(os.path.join(seg_out, "mask3d.pt"))
    assert mask3d.shape == (cfg.n_gaussians,) and mask3d.dtype == torch.bool
    run("run_pca.py", "--synthetic", "C1", "--features", path, "--max-views", "1", "--out", pca_out)
    colors = torch.load(os.path.join(pca_out, "pca_colors.pt"))["colors"]
    assert colors.shape == (cfg.n_gaussians, 3) and colors.dtype == torch.float32 and bool(torch.isfinite(colors).all())
