"""No-GPU checks of the label render: miou_recall against the reference's bookkeeping restated line by line, recolor_by_labels
against its formula, the C ABI's argument checks, and the shape of the seeded cases of tests/test_gpu_label_render.py measured on
the oracle alone (batch boundary, empty tiles, undecided share)."""
import ctypes as C

import numpy as np
import pytest
import torch

import gsbp_amd
from gsbp_amd import _lib, miou_recall, recolor_by_labels

import label_render_ref as ref


# ---- miou_recall -------------------------------------------------------------------------------------------------------------------
def _hand_made_counts():
    c = np.zeros((4, 5, 3), np.int64)
    c[0, 1] = (5, 10, 8)      # plain
    c[0, 2] = (0, 3, 0)       # predicted only: IoU 0, no recall entry (ground truth == 0)
    c[0, 3] = (0, 0, 4)       # ground truth only: IoU 0, recall 0
    c[0, 4] = (0, 0, 0)       # union == 0: skipped
    c[1, 1] = (0, 7, 9)       # intersection == 0 with both present
    c[1, 2] = (2, 2, 2)       # perfect
    c[1, 3] = (1, 5, 4)
    # view 2: a skipped view, all zero
    c[3, 0] = (50, 60, 70)    # class 0, the background: not scored by default
    c[3, 4] = (3, 3, 9)
    return c


@pytest.mark.parametrize("classes, n_present", [(None, None), (None, 3), ([0, 2, 4], None), ([1], 7)])
def test_miou_recall_reproduces_the_reference_bookkeeping(classes, n_present):
    c = _hand_made_counts()
    cls = list(range(1, c.shape[1])) if classes is None else classes
    present = sum(1 for i in cls if c[:, i, 2].sum() > 0) if n_present is None else n_present
    want = ref.bookkeeping_of_counts(c, cls, present)
    got = miou_recall(torch.from_numpy(c), classes=classes, n_present=n_present)
    assert got["n_present"] == present
    assert got["miou"] == pytest.approx(want[0], rel=1e-12) and got["mean_recall"] == pytest.approx(want[1], rel=1e-12)
    if classes is None:
        assert got["iou"][4] == pytest.approx(1.0 / 3.0) and got["recall"][2] == pytest.approx(1.0)
        assert got["iou"][3] == pytest.approx((0.0 + 1.0 / 8.0) / 2.0) and got["recall"][3] == pytest.approx(0.125)
    one_view = miou_recall(c[1])
    assert one_view["iou"][4] is None and one_view["recall"][4] is None and one_view["iou"][2] == 1.0
    assert np.isnan(miou_recall(np.zeros((2, 3, 3), np.int64))["miou"])
    with pytest.raises(gsbp_amd.GwbpError):
        miou_recall(np.zeros((2, 4), np.int64))


def test_miou_recall_equals_the_literal_loop_on_masks():
    rng = np.random.default_rng(3)
    maps = [rng.uniform(0.0, 0.6, (9, 11, 4)).astype(np.float32) for _ in range(3)]
    gts = [rng.integers(0, 4, (9, 11)), None, rng.integers(0, 3, (9, 11))]
    counts = np.stack([ref.counts_of(m, g) if g is not None else np.zeros((4, 3), np.int64) for m, g in zip(maps, gts)])
    want = ref.reference_loop(maps, gts, [1, 2, 3], 3)
    got = miou_recall(counts, n_present=3)
    assert got["miou"] == pytest.approx(want[0], rel=1e-12) and got["mean_recall"] == pytest.approx(want[1], rel=1e-12)


# ---- recolor_by_labels -------------------------------------------------------------------------------------------------------------
def test_recolor_follows_the_formula_and_scales_the_rest_once():
    g = torch.Generator().manual_seed(0)
    n = 50
    splats = dict(means=torch.rand(n, 3, generator=g), features_dc=torch.randn(n, 1, 3, generator=g),
                  features_rest=torch.randn(n, 15, 3, generator=g))
    palette = torch.tensor([[125, 125, 125], [255, 0, 0], [0, 255, 0]]) / 255.0
    labels = torch.randint(-1, 5, (n,), generator=g)
    out = recolor_by_labels(splats, labels, palette, mix=0.3, rest_scale=0.2)
    want = splats["features_dc"].clone()
    for i in range(3):
        m = labels == i
        want[m, 0] = 0.3 * want[m, 0] + 0.7 * (palette[i] - 0.5) / (1.0 / np.sqrt(4.0 * np.pi))
    assert torch.allclose(out["features_dc"], want, atol=1e-6)
    outside = (labels < 0) | (labels >= 3)
    assert outside.any() and torch.equal(out["features_dc"][outside], splats["features_dc"][outside])
    assert torch.equal(out["features_rest"], 0.2 * splats["features_rest"])   # once, not once per class
    assert out["means"] is splats["means"] and out["features_dc"] is not splats["features_dc"]
    default = recolor_by_labels(splats, labels, palette)
    assert torch.equal(default["features_rest"], 0.1 * splats["features_rest"])


# ---- the C ABI's own checks (no device call) ---------------------------------------------------------------------------------------
def test_render_labels_validates_its_own_arguments_before_the_workspace():
    L = _lib.lib()
    buf = (C.c_char * 512)()
    fake = C.c_void_p((C.addressof(buf) + 255) & ~255)
    odd = C.c_void_p(fake.value + 2)
    half = C.c_void_p(fake.value + 4)

    def call(labels=fake, k=8, maps=fake, alphas=None, argmax=None, sums=None, gt=None, cut=64, counts=None):
        return L.gwbp_render_labels(None, None, 0, None, labels, k, maps, alphas, argmax, sums, 0.0, gt, cut, counts, None)

    for kw, msg in ((dict(k=0), b"num_classes must be in"), (dict(k=-3), b"num_classes must be in"), (dict(labels=None), b"labels must be"),
                    (dict(labels=odd), b"labels must be"), (dict(maps=None), b"every output is null"),
                    (dict(maps=odd), b"4-B aligned"), (dict(k=65, argmax=fake), b"needs argmax_sums"),
                    (dict(gt=fake), b"gt and counts go together"), (dict(counts=fake), b"gt and counts go together"),
                    (dict(gt=fake, counts=half), b"counts 8-B"), (dict(cut=256), b"cut must be in"), (dict(cut=-1), b"cut must be in")):
        assert call(**kw) == -1, kw
        assert msg in L.gwbp_last_error_string(), (kw, L.gwbp_last_error_string())
    # valid own arguments get as far as the caps
    assert call(k=65, argmax=fake, sums=fake, gt=fake, counts=fake) == -1 and b"null caps" in L.gwbp_last_error_string()


# ---- the seeded cases of the GPU tests, on the oracle alone ------------------------------------------------------------------------
def test_scenes_cross_the_batch_boundary_and_leave_tiles_empty(orc):
    per_tile = {kind: np.diff(ref.front(kind, 0)[1]["tile_offsets"]) for kind in ref.SCENES}
    assert per_tile["dense"].max() > 256 and per_tile["dense"].size == 15
    assert per_tile["sparse"].min() == 0 and per_tile["sparse"].max() > 0


@pytest.mark.parametrize("kind, k", ref.CASES, ids=ref.CASE_IDS)
def test_undecided_share_of_the_gpu_cases(orc, kind, k):
    labels = ref.labels_of(kind, k)
    assert labels.min() == -1 and labels.max() >= k
    gt = ref.gt_of(kind, k, 0)
    assert gt.min() < 0 and gt.max() >= k and gt.shape == (ref.H, ref.W)
    maps, alphas = ref.oracle_maps(kind, k)
    und = ref.undecided(maps)
    touched = maps > 0
    print(f"{kind} K={k}: {int(und.sum())} of {und.size} cases undecided ({100.0 * und.mean():.4f} %), "
          f"{int(touched.sum())} with a contribution, {int(ref.predicted(maps).sum())} predicted")
    assert und.mean() <= 0.01
    assert touched.any() and float(alphas.max()) > 0.5


def test_the_score_case_has_no_undecided_case(orc):
    kind, k = ref.SCORE_CASE
    n_und = sum(int(ref.undecided(ref.oracle_maps(kind, k, v)[0])[..., 1:].sum()) for v in (0, 2))   # view 1 is skipped
    n_pred = sum(int(ref.predicted(ref.oracle_maps(kind, k, v)[0])[..., 1:].sum()) for v in (0, 2))
    print(f"score case {kind} K={k}: {n_und} undecided, {n_pred} predicted")
    assert n_und == 0 and n_pred > 50
