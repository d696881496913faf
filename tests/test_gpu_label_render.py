"""The label render on the GPU (gwbp_render_labels): maps and alphas bit for bit against the render of the one-hot table and within
1e-4 of the oracle's, the fused counts exactly against numpy on the same maps and on every decided case against the oracle's,
accumulation, class chunks, the argmax, each output alone, score_label_views + miou_recall against the reference's loop, the reuse
of a rendered view's front, and the argument errors.  Cases, scenes and seeds: tests/label_render_ref.py (their undecided share is
measured on the oracle in tests/test_label_render_cpu.py)."""
import numpy as np
import pytest
import torch

import gsbp_amd
from gsbp_amd.rasterization import get_engine

import label_render_ref as ref

pytestmark = pytest.mark.gpu
W, H = ref.W, ref.H
MIN_OPACITY = 0.3
_RUNS = {}
_FRONTS = {}


def front_of(dev, kind):
    """One engine per scene with view 0 projected and sorted: every case of the scene renders from it."""
    if kind not in _FRONTS:
        gauss, vms, K = ref.device_scene(kind, dev)
        eng = gsbp_amd.Engine(gauss[0].shape[0], W, H, device=dev)
        view = eng.view(vms[0], K, W, H)
        eng.project(view, *gauss)
        eng.bin_sort(view)
        assert not eng.stats()["overflow"]
        _FRONTS[kind] = (eng, view)
    return _FRONTS[kind]


def run_of(dev, kind, k):
    """The all-outputs call of a case (shared: nobody writes into it)."""
    if (kind, k) not in _RUNS:
        eng, view = front_of(dev, kind)
        labels = ref.device_labels(kind, k, dev)
        gt = torch.from_numpy(ref.gt_of(kind, k, 0)).to(dev)
        maps, alphas, argmax, counts = eng.render_labels(view, labels, k, want_argmax=True, gt=gt)
        _RUNS[kind, k] = dict(eng=eng, view=view, labels=labels, gt=gt, maps=maps, alphas=alphas, argmax=argmax, counts=counts)
    return _RUNS[kind, k]


# ---- 1. maps and alphas ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, k", ref.CASES, ids=ref.CASE_IDS)
def test_maps_and_alphas_equal_the_one_hot_render(dev, orc, kind, k):
    r = run_of(dev, kind, k)
    assert r["maps"].shape == (H, W, k) and r["alphas"].shape == (H, W) and r["maps"].dtype == torch.float32
    if k <= 32:
        table = torch.from_numpy(ref.one_hot(ref.labels_of(kind, k), k)).to(dev)
        want, want_alpha = r["eng"].render_pixels(r["view"], table)
        assert torch.equal(r["maps"], want) and torch.equal(r["alphas"], want_alpha)
    o_maps, o_alphas = ref.oracle_maps(kind, k)
    err = float(np.abs(r["maps"].cpu().numpy() - o_maps).max())
    err_a = float(np.abs(r["alphas"].cpu().numpy() - o_alphas).max())
    print(f"{kind} K={k}: max |maps - oracle| = {err:.2e}, alphas {err_a:.2e}")
    assert err <= 1e-4 and err_a <= 1e-4
    assert float(r["maps"].max()) > 0.2


# ---- 2. counts ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, k", ref.CASES, ids=ref.CASE_IDS)
def test_counts_equal_numpy_on_the_same_maps_and_the_oracle_on_decided_cases(dev, orc, kind, k):
    r = run_of(dev, kind, k)
    maps, gt = r["maps"].cpu().numpy(), ref.gt_of(kind, k, 0)
    assert r["counts"].dtype == torch.int64 and r["counts"].shape == (k, 3)
    assert np.array_equal(r["counts"].cpu().numpy(), ref.counts_of(maps, gt))
    assert int(r["counts"][:, 1].sum()) > 0 and int(r["counts"][:, 2].sum()) > 0
    o_maps = ref.oracle_maps(kind, k)[0]
    decided = ~ref.undecided(o_maps)
    differ = ref.predicted(maps) != ref.predicted(o_maps)
    print(f"{kind} K={k}: {int((~decided).sum())} undecided cases, {int((differ & ~decided).sum())} of them differ")
    assert not (differ & decided).any()
    if decided.all():
        assert np.array_equal(r["counts"].cpu().numpy(), ref.counts_of(o_maps, gt))


# ---- 3. accumulation and class chunks ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, k", [("dense", 8), ("sparse", 65), ("dense", 150)], ids=["dense-K8", "sparse-K65", "dense-K150"])
def test_counts_add_into_what_is_there(dev, kind, k):
    r = run_of(dev, kind, k)
    buf = torch.full((k, 3), 7, dtype=torch.int64, device=dev)
    out = r["eng"].render_labels(r["view"], r["labels"], k, want_maps=False, want_alphas=False, gt=r["gt"], counts=buf)[3]
    assert out is buf and torch.equal(buf, r["counts"] + 7)
    r["eng"].render_labels(r["view"], r["labels"], k, want_maps=False, want_alphas=False, gt=r["gt"], counts=buf)
    assert torch.equal(buf, 2 * r["counts"] + 7)


@pytest.mark.parametrize("kind, k", [("dense", 65), ("sparse", 150), ("dense", 150)], ids=["dense-K65", "sparse-K150", "dense-K150"])
def test_chunked_classes_equal_one_launch_on_a_relabelled_copy(dev, kind, k):
    r = run_of(dev, kind, k)
    for base in range(0, k, 64):
        kc = min(64, k - base)
        maps, _, _, counts = r["eng"].render_labels(r["view"], r["labels"] - base, kc, want_alphas=False, gt=r["gt"] - base)
        assert torch.equal(maps, r["maps"][..., base:base + kc]) and torch.equal(counts, r["counts"][base:base + kc])


# ---- 4. argmax ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, k", ref.CASES, ids=ref.CASE_IDS)
def test_argmax_takes_the_lowest_index_and_minus_one_below_min_opacity(dev, kind, k):
    r = run_of(dev, kind, k)
    maps = r["maps"].cpu().numpy()
    best = maps.max(axis=-1)
    want = maps.argmax(axis=-1).astype(np.int32)   # numpy: the first of equals
    want[best <= 0] = -1
    assert r["argmax"].dtype == torch.int32 and np.array_equal(r["argmax"].cpu().numpy(), want)
    assert (want >= 0).any() and (kind == "dense" or (want == -1).any())
    got = r["eng"].render_labels(r["view"], r["labels"], k, want_maps=False, want_alphas=False, want_argmax=True,
                                 min_opacity=MIN_OPACITY)[2]
    want[best < MIN_OPACITY] = -1
    assert np.array_equal(got.cpu().numpy(), want) and (want >= 0).any()


def test_argmax_across_a_chunk_boundary(dev):
    """Two classes only, one in each chunk of a 65-class table (3 and 64, by the Gaussian's parity): the running (sum, class) pair
    carried from the first chunk into the second decides every pixel as the two maps do, the lower index where they are equal."""
    gauss, vms, K = ref.device_scene("dense", dev)
    r = run_of(dev, "dense", 65)
    labels = torch.where(torch.arange(gauss[0].shape[0], device=dev) % 2 == 0, 3, 64).to(torch.int32)
    maps, _, argmax, _ = r["eng"].render_labels(r["view"], labels, 65, want_argmax=True)
    a, b = maps[..., 3], maps[..., 64]
    want = torch.where(a >= b, 3, 64).to(torch.int32)
    want[(a <= 0) & (b <= 0)] = -1
    assert torch.equal(argmax, want) and bool((want == 3).any()) and bool((want == 64).any())


# ---- 5. each output alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, k", [("dense", 8), ("sparse", 33), ("dense", 65)], ids=["dense-K8", "sparse-K33", "dense-K65"])
def test_each_output_alone_equals_the_all_outputs_call(dev, kind, k):
    r = run_of(dev, kind, k)
    eng, view, labels = r["eng"], r["view"], r["labels"]
    maps, alphas, argmax, counts = eng.render_labels(view, labels, k, want_alphas=False)
    assert torch.equal(maps, r["maps"]) and alphas is None and argmax is None and counts is None
    maps, alphas, argmax, counts = eng.render_labels(view, labels, k, want_maps=False)
    assert maps is None and torch.equal(alphas, r["alphas"]) and argmax is None and counts is None
    maps, alphas, argmax, counts = eng.render_labels(view, labels, k, want_maps=False, want_alphas=False, want_argmax=True)
    assert maps is None and alphas is None and torch.equal(argmax, r["argmax"]) and counts is None
    maps, alphas, argmax, counts = eng.render_labels(view, labels, k, want_maps=False, want_alphas=False, gt=r["gt"])
    assert maps is None and alphas is None and argmax is None and torch.equal(counts, r["counts"])
    # int64 labels and ground truth are narrowed, with the same result
    wide = eng.render_labels(view, labels.long(), k, want_maps=False, want_alphas=False, gt=r["gt"].long())[3]
    assert torch.equal(wide, r["counts"])


# ---- 6. score_label_views and miou_recall ------------------------------------------------------------------------------------------
def test_scored_views_give_the_reference_loops_miou_and_recall(dev, orc):
    kind, k = ref.SCORE_CASE
    gauss, vms, K = ref.device_scene(kind, dev)
    labels = ref.device_labels(kind, k, dev)
    gts = [ref.gt_of(kind, k, 0), None, ref.gt_of(kind, k, 2)]
    counts = gsbp_amd.score_label_views(*gauss, labels, k, vms, K, W, H,
                                        lambda v: None if gts[v] is None else torch.from_numpy(gts[v]).to(dev))
    assert counts.shape == (3, k, 3) and counts.dtype == torch.int64 and not bool(counts[1].any())
    o_maps = [ref.oracle_maps(kind, k, v)[0] for v in range(3)]
    for v in (0, 2):   # no scored case is undecided (test_label_render_cpu): the counts are the oracle's
        assert np.array_equal(counts[v, 1:].cpu().numpy(), ref.counts_of(o_maps[v], gts[v])[1:])
    classes = list(range(1, k))
    n_present = sum(1 for i in classes if any(g is not None and (g == i).any() for g in gts))
    want = ref.reference_loop(o_maps, gts, classes, n_present)
    got = gsbp_amd.miou_recall(counts)
    print(f"mIoU {got['miou']:.6f} (reference loop {want[0]:.6f}), recall {got['mean_recall']:.6f} ({want[1]:.6f})")
    assert got["n_present"] == n_present
    assert got["miou"] == pytest.approx(want[0], rel=1e-12) and got["mean_recall"] == pytest.approx(want[1], rel=1e-12)
    # the reference's own divisor: the distinct labels of the last view minus one
    last = np.unique(gts[2]).size - 1
    assert gsbp_amd.miou_recall(counts, n_present=last)["miou"] == pytest.approx(ref.reference_loop(o_maps, gts, classes, last)[0], rel=1e-12)


# ---- 7. the front of a rendered view is reused -------------------------------------------------------------------------------------
def test_label_render_after_a_rendered_frame_projects_nothing(dev):
    kind, k = "dense", 8
    gauss, vms, K = ref.device_scene(kind, dev)
    labels = ref.device_labels(kind, k, dev)
    colors = torch.rand(gauss[0].shape[0], 3, generator=torch.Generator().manual_seed(1)).to(dev)
    with torch.no_grad():
        gsbp_amd.rasterization(*gauss, colors, vms[:1], K[None], W, H, want_meta=False)
    eng = get_engine(dev, gauss[0].shape[0], W, H)
    gen = eng.generation
    maps, alphas = gsbp_amd.render_label_maps(*gauss, labels, k, vms[0], K, W, H)
    seg = gsbp_amd.render_label_argmax(*gauss, labels, k, vms[0], K, W, H)
    assert eng.generation == gen, "the label render re-projected a view the workspace already held"
    r = run_of(dev, kind, k)
    assert torch.equal(maps, r["maps"]) and torch.equal(alphas, r["alphas"]) and torch.equal(seg, r["argmax"])
    gsbp_amd.render_label_argmax(*gauss, labels, k, vms[1], K, W, H)
    assert eng.generation == gen + 1
    with pytest.raises(TypeError):
        gsbp_amd.render_label_maps(*gauss, labels, k, vms[0], K, W, H, sh_degree=3)


# ---- 8. argument errors ------------------------------------------------------------------------------------------------------------
def test_argument_errors_raise_with_a_message_and_leave_the_device_usable(dev):
    r = run_of(dev, "sparse", 8)
    eng, view, labels, gt = r["eng"], r["view"], r["labels"], r["gt"]
    for kw, msg in ((dict(labels=labels.float()), "integer"), (dict(labels=labels.cpu()), "device"),
                    (dict(labels=labels[:-1]), "Gaussians"), (dict(k=0), "num_classes"), (dict(k=-2), "num_classes"),
                    (dict(gt=gt[:-1]), r"\[H,W\]"), (dict(gt=gt.float()), "integer"),
                    (dict(gt=gt, counts=torch.zeros(7, 3, dtype=torch.int64, device=dev)), r"\[8,3\]"),
                    (dict(gt=gt, counts=torch.zeros(8, 3, dtype=torch.int32, device=dev)), "int64"),
                    (dict(counts=torch.zeros(8, 3, dtype=torch.int64, device=dev)), "ground-truth"),
                    (dict(gt=gt, cut=256), "cut must be in"), (dict(want_maps=False, want_alphas=False), "no output")):
        kw = dict(dict(labels=labels, k=8), **kw)
        lab, k = kw.pop("labels"), kw.pop("k")
        with pytest.raises(gsbp_amd.GwbpError, match=msg):
            eng.render_labels(view, lab, k, **kw)
    with pytest.raises(gsbp_amd.GwbpError, match="HIP tensors"):
        gsbp_amd.render_label_maps(*(t.cpu() for t in ref.scene("sparse")[0]), labels.cpu(), 8, ref.scene("sparse")[1][0],
                                   ref.scene("sparse")[2], W, H)
    again = eng.render_labels(view, labels, 8, want_argmax=True, gt=gt)
    assert torch.equal(again[0], r["maps"]) and torch.equal(again[3], r["counts"])
