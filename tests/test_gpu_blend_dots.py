"""The dots kernel ALONE (k_render_dots_bwd through Engine.render_dots_backward / gwbp_render_dots_backward) against the list-based
float64 yardstick of tests/blend_grad_ref.py, fed the SAME float32 records, tile lists and set of valid pairs the kernel read -- the
fronts, the seeded data and the figure code are those of tests/test_gpu_blend_grad.py.

    channels       D in {1, 64, 65, 128}: both sides of the edge between the two instantiations (CH = 64, 128), and the ends
    row stride     D = 65 as a [:, :65] view of an [N, 160] table whose other columns hold NaN
    alpha          v_alpha = None; v_out = 0 beside a random v_alpha
    list lengths   one tile's list of 1, 32, 33, 64, 65, 256, 257, 513 records, nobody terminating: 64 is the kernel's batch of pass 2
                   (kDotBatch), 256 the batch of pass 1
    termination    600 records, every pixel ending somewhere else, n_used inside the 2nd / 3rd batch of pass 1
    tile counts    256 and 272 tiles: 1 and 2 passes of the tile sort, the sorted lists in buffer 1 and 0
    added into     two calls into the same v_g2d; rows without a pair keep their bits
    non-finite     NaN colours of Gaussians that contribute nowhere reach nothing; NaN colours of valid pairs stay at their pixels

The kernel has no colour gradient (it is Engine.scatter's, tests/test_gpu_latent_render.py): the rule's 15 figures of v_g2d are judged,
as test_gpu_blend_grad.py judges a want_colors=False call.  Rule: kernel <= FACTOR x the float32 run of the same reference, per
quantity, figure and case.  FACTOR = the largest kernel / floor ratio measured on an MI355X over every case below
(tools/record_blend_dots.py -> profiles/blend_dots.json), times 2, rounded up; above 16 it would not have been accepted.
"""
from ctypes import byref, c_int64

import pytest
import torch

import blend_grad_ref as bg
import front_boundary_scenes as fb
from gsbp_amd._lib import ptr
from gsbp_amd.engine import row_stride
from test_gpu_blend_grad import T0, _nan_split, data, front

pytestmark = pytest.mark.gpu
# Measured on an MI355X (profiles/blend_dots.json: 24 comparisons, 360 figures).  Floors: 3.0e-8 .. 4.9e-7 Frobenius-relative, up to
# 7.5e-7 max-abs, 5.2e-8 .. 6.5e-5 per row; the kernel: 8.7e-9 .. 1.1e-7, up to 1.6e-7, 9.3e-9 .. 3.4e-5 per row.  kernel / floor: median
# 0.21 (Frobenius), 0.24 (max-abs), 0.11 (row).  Largest: 3.74, the cb column of the one-record list -- one Gaussian in one tile, so the
# figure is the rounding of a single float32 number and the same in every run: the kernel's is 1.12e-7 (one ulp), the float32
# reference's happens to be 2.98e-8 (a quarter of an ulp).  Next: 1.00 (the cc column of the same list: the same float32 number on both
# sides), then 0.93.  ceil(2 x 3.74) = 8, below the ceiling of 16.  (With float32 arithmetic behind the rows the same figure stood at
# 9.97, which the rule does not accept: the kernel computes everything behind its float32 inputs in float64 since)
FACTOR = 8.0
DOT_BATCH = 64  # kDotBatch of csrc/render_grad_wide.hip
CHANNELS = (1, 64, 65, 128)
LIST_LENGTHS = (1, 32, 33, DOT_BATCH, DOT_BATCH + 1, 256, 257, 513)
ROWS = []  # every figure of every comparison of this process, in order (tools/record_blend_dots.py files them)


def backward(dev, key, D, variant="seeded", table=None):
    """Engine.render_dots_backward of the case -> v_g2d on the CPU."""
    f, d = front(dev, key), data(dev, key, D, variant)
    table = d["table"].to(dev) if table is None else table
    v_alpha = None if d["v_alpha"] is None else d["v_alpha"].to(dev)
    return f["eng"].render_dots_backward(f["view"], table, d["v_out"].to(dev), v_alpha).cpu()


def compare(name, v_g2d, d):
    rows = bg.report(name, (v_g2d, None), d["truth"], d["floor"])
    bg.show(rows)
    ROWS.extend(rows)
    assert len(rows) == 15
    return rows


def check(rows):
    assert rows and not bg.failures(rows, FACTOR), bg.failures(rows, FACTOR)


def consistent(dev, key, D, variant="seeded"):
    """Cut, lists and records belong together: the reference's float64 render agrees with Engine.render (the weight store the front's
    blend left; render_pixels stops at 32 channels) of the same view to 1e-5."""
    f, d = front(dev, key), data(dev, key, D, variant)
    image = f["eng"].render(f["view"], d["colors"].to(dev))
    e_out = float((image.cpu().double() - d["truth"]["out"]).abs().max())
    assert float(d["truth"]["alpha_img"].max()) > 0.01 and e_out <= 1e-5, (key, e_out)


def run(dev, name, key, D, variant="seeded"):
    consistent(dev, key, D, variant)
    check(compare(name, backward(dev, key, D, variant), data(dev, key, D, variant)))


@pytest.mark.parametrize("D", CHANNELS)
def test_channel_edges(dev, D):
    run(dev, f"dots-channels-{D}", T0, D)


def test_antialiased_records(dev):
    run(dev, "dots-antialiased", ("t0", "antialiased"), 33)


def test_row_stride_above_the_channel_count(dev):
    """ldc = 160 > D = 65, NaN in the columns the kernel must not read."""
    d = data(dev, T0, 65)
    wide = torch.full((d["colors"].shape[0], 160), float("nan"), device=dev)
    wide[:, :65] = d["colors"].to(dev)
    table = wide[:, :65]
    assert row_stride(table) == 160 and not table.is_contiguous()
    v_g2d = backward(dev, T0, 65, table=table)
    assert bool(torch.isfinite(v_g2d).all())
    check(compare("dots-stride-160-D65", v_g2d, d))


def test_without_v_alpha(dev):
    assert data(dev, T0, 33, "no-alpha")["v_alpha"] is None
    run(dev, "dots-no-v_alpha", T0, 33, "no-alpha")


def test_v_alpha_alone(dev):
    d = data(dev, T0, 33, "zero-out")
    assert float(d["truth"]["v_g2d"].abs().max()) > 0
    run(dev, "dots-v_alpha-alone", T0, 33, "zero-out")


@pytest.mark.parametrize("n", LIST_LENGTHS)
def test_list_lengths_around_both_batch_sizes(dev, n):
    """One tile's list of n records at opacity 0.02: nobody terminates, so n_used = n and pass 2 starts with a last batch of n % 64."""
    key = ("stack", 0.02, n)
    f, d = front(dev, key), data(dev, key, 33)
    assert bg.list_length(f["plan"], bg.STACK_TILE) == n
    assert bg.nobody_terminates(d["truth"], 0.02)
    assert int(bg.last_positions(f["plan"], bg.STACK_TILE).max()) == n - 1  # somebody takes the list's last record
    run(dev, f"dots-list-{n}", key, 33)


@pytest.mark.parametrize("opacity", bg.TERMINATION_OPACITIES)
def test_termination_past_the_first_batch(dev, opacity):
    key = ("stack", opacity, 600)
    f = front(dev, key)
    lo, hi, kinds = bg.check_termination(f["plan"])
    assert (hi - 1) // 256 == (2 if opacity == 0.15 else 1)
    unpaired = ~f["plan"]["paired"]
    assert int(unpaired.sum()) >= 1
    v_g2d = backward(dev, key, 128)
    assert not v_g2d[unpaired].any()
    check(compare(f"dots-termination-{opacity}", v_g2d, data(dev, key, 128)))


@pytest.mark.parametrize("name", ["t256", "t272"])
def test_tile_counts_on_both_parities_of_the_sort_buffer(dev, name):
    key = ("tiles", name)
    f = front(dev, key)
    nt = fb.n_tiles(f["W"], f["H"])
    assert fb.sort_passes(nt) == {"t256": 1, "t272": 2}[name]
    run(dev, f"dots-tiles-{name}", key, 65)


def _call(f, table, v_out, v_alpha, v_g2d):
    eng, D = f["eng"], table.shape[1]
    eng._call("gwbp_render_dots_backward", *eng._args(), byref(f["view"]), ptr(table), c_int64(row_stride(table)), D, ptr(v_out),
              ptr(v_alpha), ptr(v_g2d), eng._stream())


def test_v_g2d_is_added_into(dev):
    f, d = front(dev, T0), data(dev, T0, 65)
    args = [d["table"].to(dev), d["v_out"].to(dev), d["v_alpha"].to(dev)]
    v_g2d = torch.zeros(f["n"], 6, device=dev)
    _call(f, *args, v_g2d)
    _call(f, *args, v_g2d)
    check(compare("dots-added-twice", 0.5 * v_g2d.cpu(), d))  # (halving is exact)
    unpaired = (~f["plan"]["paired"]).to(dev)
    assert int(unpaired.sum()) >= 10
    v_g2d = torch.zeros(f["n"], 6, device=dev)
    v_g2d[unpaired] = 1.0
    _call(f, *args, v_g2d)
    assert bool((v_g2d[unpaired] == 1.0).all())
    v_g2d[unpaired] = 0.0
    check(compare("dots-added-prefilled", v_g2d.cpu(), d))


def test_non_finite_colours_of_unpaired_gaussians_reach_nothing(dev):
    """The opacity-0.6 stack: the Gaussians behind the dozen records every pixel takes lie in the batches pass 2 stages, with NaN colours."""
    key = ("stack", 0.6, 600)
    f, d = front(dev, key), data(dev, key, 65, "nan")
    unpaired = ~f["plan"]["paired"]
    assert int(unpaired.sum()) >= 50 and bool(torch.isnan(d["table"][unpaired]).all())
    v_g2d = backward(dev, key, 65, "nan")
    assert bool(torch.isfinite(v_g2d).all()) and not v_g2d[unpaired].any()
    check(compare("dots-nan-colours", v_g2d, d))


def test_non_finite_colours_of_valid_pairs_stay_at_their_pixels(dev):
    """Every 16th Gaussian of T0 has a NaN row AND valid pairs: m_j is NaN in every lane of a wave that reads the row, and the selects
    must keep it from the lanes where the pair is not valid and from the B of the pixels that do not take it."""
    f, d = front(dev, T0), data(dev, T0, 65)
    pl = f["plan"]
    nan_rows = pl["paired"] & (torch.arange(f["n"]) % 16 == 0)
    clean, exposed = _nan_split(pl, nan_rows)
    assert int(nan_rows.sum()) >= 20 and int(clean.sum()) >= 40 and exposed >= 20
    table = torch.where(nan_rows[:, None], torch.full_like(d["colors"], float("nan")), d["colors"])
    v_g2d = f["eng"].render_dots_backward(f["view"], table.to(dev), d["v_out"].to(dev), d["v_alpha"].to(dev)).cpu()
    assert bool(torch.isnan(v_g2d[nan_rows]).any()) and bool(torch.isfinite(v_g2d[clean]).all())
    rows_of = {k: dict(v_g2d=d[k]["v_g2d"][clean], v_colors=d[k]["v_colors"][clean]) for k in ("truth", "floor")}
    check(compare("dots-nan-valid", v_g2d[clean], rows_of))
