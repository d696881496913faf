"""The blend backward kernel ALONE (k_render_px_bwd through Engine.render_pixels_backward / gwbp_render_pixels_backward) against the
list-based float64 yardstick of tests/blend_grad_ref.py, fed the SAME float32 records, tile lists and set of valid pairs the kernel
read: project -> bin_sort -> blend_weights + dump_pairs (the cut) -> render_pixels_backward.  tests/test_gpu_raster_grad.py and
tests/test_gpu_camera_grad.py see this kernel only through rasterization(): behind the projection's chain rule, with the rounding of
the projected records as their floor, on at most 24 tiles.  Here record rounding is on neither side, so each of the six columns of
v_g2d is judged on its own, and the reference skips empty tiles, so it reaches the images of 272 .. 80 000 tiles whose sorted lists
end in the other buffer (fin = sort_passes & 1).

    baseline       T0 view 0, D = 3, classic and antialiased (the filed opacity is opacity x compensation)
    channels       D in {1, 4, 5, 16, 17, 32}: both sides of each CH instantiation; with and without v_colors
    row stride     D = 5 and 32 as a [:, :D] view of an [N, 40] table whose other columns hold NaN
    alpha          v_alpha = None; v_out = 0 beside a random v_alpha
    list lengths   one tile's list of 1, 32, 33, 256, 257, 512, 513 records, nobody terminating: the sub-batch (32) and batch (256) edges
    termination    600 records, every pixel ending somewhere else, before and behind position 256; n_used inside the 2nd / 3rd batch
    tile counts    256, 272, 65 536, 80 000 tiles: 1, 2, 2, 3 passes of the tile sort
    added into     two calls into the same outputs; rows without a pair keep what they held
    non-finite     NaN colours of Gaussians that contribute nowhere reach nothing

Every case first asserts that the reference's float64 render and alpha map agree with Engine.render_pixels of the same view to 1e-5
absolute: cut, lists and records belong together.  Every condition on a scene (pass counts, list lengths, last positions) is asserted
from the kernel's own lists and cut.

Tolerance.  Per case, seven quantities (the six columns of v_g2d, and v_colors) x two figures (Frobenius-relative; max-abs over the
truth's max-abs), and a row figure (largest per-row error over max(|truth row|, 1e-3 x the largest row norm)) for the mean, conic and
opacity columns and for v_colors: 18 figures, each against the same figure of the float32 run of the SAME reference from the same
records (the floor, never the kernel).  Rule: kernel <= FACTOR x floor, per quantity, figure and case.  FACTOR = the largest
kernel / floor ratio measured on an MI355X over every case below (tools/record_blend_grad.py -> profiles/blend_grad.json), times 2 --
for what the floor does not have: the atomics' order, which differs from run to run, and exp_neg against torch.exp -- rounded up to
the next integer; above 16 it would not have been accepted.  A dropped record, a wrong sign or a missing 1/2 is off by 1e-3 .. 1 against
floors near 1e-7 .. 1e-6: tests/test_blend_grad_ref_cpu.py shows that such outputs fail at this factor, and at 16.
"""
import functools
from ctypes import byref, c_int64

import pytest
import torch

import blend_grad_ref as bg
import front_boundary_scenes as fb
import gsbp_amd
from gsbp_amd._lib import ptr
from gsbp_amd.engine import row_stride
from test_gpu_raster_grad import _stack, _t0

pytestmark = pytest.mark.gpu
# Measured on an MI355X (profiles/blend_grad.json: 35 comparisons, 612 figures, the same in three runs).  Floors: 4.6e-9 .. 9.0e-7
# Frobenius-relative, up to 1.4e-6 max-abs, 2.5e-8 .. 1.6e-4 per row; the kernel: 4.6e-9 .. 7.7e-7, up to 7.7e-7, 2.5e-8 .. 1.1e-4.
# kernel / floor: median 0.86 (Frobenius), 0.82 (max-abs), 0.70 (row).  Largest: 6.13, the cb column of the one-record list -- one
# Gaussian, so each figure is the rounding of a single float32 number: the kernel's is 7.6e-8 (0.64 ulp), the float32 reference's
# happens to be 1.2e-8.  Next: 4.57 (max-abs of the ca column at D = 16: 6.0e-7 against 1.3e-7) and 3.06 (opacity rows, D = 16).
# ceil(2 x 6.13) = 13, below the ceiling of 16.  No case exposed an error of the kernel.
FACTOR = 13.0
LIST_LENGTHS = (1, 32, 33, 256, 257, 512, 513)
ROWS = []  # every figure of every comparison of this process, in order (tools/record_blend_grad.py files them)


# ---- the kernels' side: records, lists, cut ----------------------------------------------------------------------------------------
def _scene(key):
    """key -> dict(g = (means, quats, scales, opac) float32 CPU, vm, K, W, H, view_kw, caps)."""
    if key[0] == "t0":
        s = _t0()
        return dict(g=s["inputs"][:4], vm=s["vm"], K=s["K"], W=s["W"], H=s["H"], view_kw=dict(rasterize_mode=key[1]), caps={})
    if key[0] == "stack":
        s = _stack(key[1], n=key[2])
        return dict(g=s["inputs"][:4], vm=s["vm"], K=s["K"], W=s["W"], H=s["H"], view_kw={}, caps={})
    sc = fb.tile_scene(key[1])
    # (the default pair_cap is 128 x W x H entries; a tile that stores anything takes a 1024-entry page of its shard)
    caps = dict(isect_cap=1 << 15, pair_cap=1 << 24) if sc["H"] == 17 else {}
    return dict(g=tuple(torch.from_numpy(sc[k]) for k in ("means", "quats", "scales", "opac")), vm=torch.from_numpy(sc["viewmat"]),
                K=torch.from_numpy(sc["K"]), W=sc["W"], H=sc["H"], view_kw={}, caps=caps)


@functools.lru_cache(maxsize=None)
def front(dev, key):
    """One engine per scene, projected, sorted and blended (growing on overflow as raster_grad_ref.kernel_cut does), with what the
    kernels filed: the float32 records, the tile lists and the valid pairs, as the reference's plan.  Shared; nobody writes into it."""
    sc = _scene(key)
    n, W, H = sc["g"][0].shape[0], sc["W"], sc["H"]
    eng = gsbp_amd.Engine(n, W, H, device=dev, **sc["caps"])
    view = eng.view(sc["vm"], sc["K"], W, H, **sc["view_kw"])
    g = [t.to(dev, torch.float32).contiguous() for t in sc["g"]]
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
    opa = g[3] * proj["compensations"] if "compensations" in proj else g[3]  # (float32, as k_project files it)
    # a culled row's outputs are not written: zeros, so that nothing uninitialised enters the reference's gathers
    rec = [torch.where(vis.reshape(-1, *[1] * (t.dim() - 1)), t, torch.zeros_like(t)).cpu() for t in (proj["means2d"], proj["conics"], opa)]
    pl = bg.plan(bins["flatten_ids"][:st["n_isect"]].cpu(), bins["tile_offsets"].cpu(), gid.cpu(), pix.cpu(), W, H, n)
    assert int(bins["tile_offsets"][-1]) == st["n_isect"] and len(gid) == st["n_pairs"] > 0
    return dict(eng=eng, view=view, n=n, W=W, H=H, rec=rec, plan=pl, stats=st, opac=sc["g"][3])


@functools.lru_cache(maxsize=None)
def data(dev, key, D, variant="seeded"):
    """Colour table, v_out, v_alpha (CPU) of one case and the reference's float64 and float32 runs; computed once, never modified.
    variants: "seeded"; "no-alpha" (v_alpha None); "zero-out" (v_out = 0); "nan" (NaN colours on the unpaired Gaussians: the table the
    kernel gets; the reference reads zeros there)."""
    f = front(dev, key)
    g = torch.Generator().manual_seed(7 + D)
    colors = torch.rand(f["n"], D, generator=g)
    v_out = torch.randn(f["H"], f["W"], D, generator=g)
    v_alpha = torch.randn(f["H"], f["W"], generator=g)
    table = colors
    if variant == "no-alpha":
        v_alpha = None
    elif variant == "zero-out":
        v_out = torch.zeros_like(v_out)
    elif variant == "nan":
        table = torch.where(f["plan"]["paired"][:, None], colors, torch.full_like(colors, float("nan")))
        colors = torch.where(f["plan"]["paired"][:, None], colors, torch.zeros_like(colors))
    truth = bg.blend(torch.float64, f["plan"], *f["rec"], colors, v_out, v_alpha)
    floor = bg.blend(torch.float32, f["plan"], *f["rec"], colors, v_out, v_alpha)
    return dict(colors=colors, table=table, v_out=v_out, v_alpha=v_alpha, truth=truth, floor=floor)


def consistent(dev, key, D, variant="seeded"):
    """The consistency assertion: the reference's float64 render agrees with Engine.render_pixels of the same view to 1e-5."""
    f, d = front(dev, key), data(dev, key, D, variant)
    image, alphas = f["eng"].render_pixels(f["view"], d["colors"].to(dev))
    e_out = float((image.cpu().double() - d["truth"]["out"]).abs().max())
    e_alpha = float((alphas.cpu().double() - d["truth"]["alpha_img"]).abs().max())
    assert float(d["truth"]["alpha_img"].max()) > 0.01  # (a single record of opacity 0.02 reaches 0.02)
    assert e_out <= 1e-5 and e_alpha <= 1e-5, (key, e_out, e_alpha)


def backward(dev, key, D, variant="seeded", want_colors=True, table=None):
    """Engine.render_pixels_backward of the case -> (v_g2d, v_colors or None) on the CPU."""
    f, d = front(dev, key), data(dev, key, D, variant)
    table = d["table"].to(dev) if table is None else table
    v_alpha = None if d["v_alpha"] is None else d["v_alpha"].to(dev)
    v_colors, v_g2d = f["eng"].render_pixels_backward(f["view"], table, d["v_out"].to(dev), v_alpha, want_colors)
    assert (v_colors is None) == (not want_colors)
    return v_g2d.cpu(), None if v_colors is None else v_colors.cpu()


def compare(name, kernel, d):
    rows = bg.report(name, kernel, d["truth"], d["floor"])
    bg.show(rows)
    ROWS.extend(rows)
    return rows


def check(rows):
    assert rows and not bg.failures(rows, FACTOR), bg.failures(rows, FACTOR)


def run(dev, name, key, D, variant="seeded", want_colors=True):
    consistent(dev, key, D, variant)
    rows = compare(name, backward(dev, key, D, variant, want_colors), data(dev, key, D, variant))
    check(rows)
    return rows


T0 = ("t0", "classic")


# ---- the tests -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["classic", "antialiased"])
def test_baseline(dev, mode):
    f = front(dev, ("t0", mode))
    assert len(f["plan"]["batches"]) >= 1 and int(f["plan"]["paired"].sum()) > 300
    if mode == "antialiased":  # the filed opacity is not the input's
        assert not torch.equal(f["rec"][2][f["plan"]["paired"]], f["opac"][f["plan"]["paired"]])
    assert len(run(dev, f"t0-{mode}", ("t0", mode), 3)) == 18


@pytest.mark.parametrize("want_colors", [True, False], ids=["colors", "no-colors"])
@pytest.mark.parametrize("D", [1, 4, 5, 16, 17, 32])
def test_channel_edges(dev, D, want_colors):
    rows = run(dev, f"channels-{D}-{'colors' if want_colors else 'no-colors'}", T0, D, want_colors=want_colors)
    assert len(rows) == (18 if want_colors else 15)


@pytest.mark.parametrize("D", [5, 32])
def test_row_stride_above_the_channel_count(dev, D):
    """ldc = 40 > D, NaN in the columns the kernel must not read."""
    d = data(dev, T0, D)
    wide = torch.full((d["colors"].shape[0], 40), float("nan"), device=dev)
    wide[:, :D] = d["colors"].to(dev)
    table = wide[:, :D]
    assert row_stride(table) == 40 and not table.is_contiguous()
    consistent(dev, T0, D)
    v_g2d, v_colors = backward(dev, T0, D, table=table)
    assert bool(torch.isfinite(v_g2d).all()) and bool(torch.isfinite(v_colors).all())
    check(compare(f"stride-40-D{D}", (v_g2d, v_colors), d))


def test_without_v_alpha(dev):
    """v_alpha = nullptr is v_alpha = 0."""
    assert data(dev, T0, 3, "no-alpha")["v_alpha"] is None
    run(dev, "no-v_alpha", T0, 3, "no-alpha")


def test_v_alpha_alone(dev):
    """v_out = 0: the colour gradient is exactly zero, and v_g2d carries the alpha map's term alone."""
    d = data(dev, T0, 3, "zero-out")
    assert float(d["truth"]["v_g2d"].abs().max()) > 0 and not d["truth"]["v_colors"].any()
    consistent(dev, T0, 3, "zero-out")
    v_g2d, v_colors = backward(dev, T0, 3, "zero-out")
    assert not v_colors.any()
    check(compare("v_alpha-alone", (v_g2d, v_colors), d))


@pytest.mark.parametrize("n", LIST_LENGTHS)
def test_list_lengths_around_the_sub_batch_and_the_batch(dev, n):
    """One tile's list of n records at opacity 0.02: nobody terminates, so n_used = n and pass 2 starts with a last batch of
    n % 256 and a last sub-batch of n % 32 records (1, 32, 33, 256, 257, 512, 513: 1 and 32 records on either side of each edge)."""
    key = ("stack", 0.02, n)
    f, d = front(dev, key), data(dev, key, 3)
    assert bg.list_length(f["plan"], bg.STACK_TILE) == n
    assert bg.nobody_terminates(d["truth"], 0.02)
    assert int(bg.last_positions(f["plan"], bg.STACK_TILE).max()) == n - 1  # somebody takes the list's last record
    run(dev, f"list-{n}", key, 3)


@pytest.mark.parametrize("opacity", bg.TERMINATION_OPACITIES)
def test_termination_past_the_first_batch(dev, opacity):
    """600 records; the tile's pixels end at many different positions on both sides of the first batch, the last of them inside the
    third batch (opacity 0.15) or the second (0.2): nothing behind a pixel's last record may receive anything from it, and a
    Gaussian no pixel takes gets exact zero rows."""
    key = ("stack", opacity, 600)
    f = front(dev, key)
    lo, hi, kinds = bg.check_termination(f["plan"])
    print(f"opacity {opacity}: last positions {lo} .. {hi} (from 1), {kinds} different")
    assert (hi - 1) // 256 == (2 if opacity == 0.15 else 1)
    unpaired = ~f["plan"]["paired"]
    assert int(unpaired.sum()) >= 1
    consistent(dev, key, 3)
    v_g2d, v_colors = backward(dev, key, 3)
    assert not v_g2d[unpaired].any() and not v_colors[unpaired].any()
    check(compare(f"termination-{opacity}", (v_g2d, v_colors), data(dev, key, 3)))


@pytest.mark.parametrize("name", ["t256", "t272", "t65536", "t80000"])
def test_tile_counts_at_every_pass_count_of_the_tile_sort(dev, name):
    """1, 2, 2 and 3 byte-passes: the sorted lists end in buffer 1, 0, 0 and 1 (launch_render_px_bwd's fin)."""
    key = ("tiles", name)
    f, d = front(dev, key), data(dev, key, 3)
    nt = fb.n_tiles(f["W"], f["H"])
    assert fb.sort_passes(nt) == fb.TILE_PASSES[name] == {"t256": 1, "t272": 2, "t65536": 2, "t80000": 3}[name]
    filled = torch.cat([bt["tiles"] for bt in f["plan"]["batches"]])
    assert int(filled.min()) < 256 and int(filled.max()) >= nt - nt // 4  # the lists spread over the tile ids
    paired = f["plan"]["paired"]
    assert int(paired.sum()) >= 0.9 * f["n"]
    assert bool(d["truth"]["v_g2d"][paired].abs().sum(dim=1).gt(0).all()) and bool(d["truth"]["v_colors"][paired].abs().sum(dim=1).gt(0).all())
    if name == "t80000":  # the Gaussians forced into tile ids that differ in the third byte only, and their partners
        assert bool(paired[:2 * fb.PAIRED].all())
        assert int(filled.max()) >= 65536 + 256
    run(dev, f"tiles-{name}", key, 3)


def _call_backward(f, table, v_out, v_alpha, v_colors, v_g2d):
    """gwbp_render_pixels_backward as Engine.render_pixels_backward issues it, into outputs of the caller's."""
    eng, D = f["eng"], table.shape[1]
    eng._call("gwbp_render_pixels_backward", *eng._args(), byref(f["view"]), ptr(table), c_int64(row_stride(table)), D, ptr(v_out),
              ptr(v_alpha), ptr(v_colors), ptr(v_g2d), eng._stream())


def test_outputs_are_added_into(dev):
    f, d = front(dev, T0), data(dev, T0, 3)
    consistent(dev, T0, 3)
    args = [d["table"].to(dev), d["v_out"].to(dev), d["v_alpha"].to(dev)]
    v_g2d, v_colors = torch.zeros(f["n"], 6, device=dev), torch.zeros(f["n"], 3, device=dev)
    _call_backward(f, *args, v_colors, v_g2d)
    _call_backward(f, *args, v_colors, v_g2d)
    check(compare("added-twice", (0.5 * v_g2d.cpu(), 0.5 * v_colors.cpu()), d))  # (halving is exact)
    unpaired = (~f["plan"]["paired"]).to(dev)
    assert int(unpaired.sum()) >= 10  # (T0, view 0: the culled Gaussians and a few that reach no pixel)
    v_g2d, v_colors = torch.zeros(f["n"], 6, device=dev), torch.zeros(f["n"], 3, device=dev)
    v_g2d[unpaired], v_colors[unpaired] = 1.0, 1.0
    _call_backward(f, *args, v_colors, v_g2d)
    assert bool((v_g2d[unpaired] == 1.0).all()) and bool((v_colors[unpaired] == 1.0).all())
    v_g2d[unpaired], v_colors[unpaired] = 0.0, 0.0
    check(compare("added-prefilled", (v_g2d.cpu(), v_colors.cpu()), d))


def test_non_finite_colours_reach_only_valid_pairs(dev):
    """The opacity-0.6 stack: every pixel terminates after a dozen records, and the Gaussians behind contribute nowhere -- but lie in
    the tile's list, inside the batch pass 2 stages.  Their colours are NaN."""
    key = ("stack", 0.6, 600)
    f, d = front(dev, key), data(dev, key, 3, "nan")
    unpaired = ~f["plan"]["paired"]
    assert int(unpaired.sum()) >= 50 and bool(torch.isnan(d["table"][unpaired]).all()) and bool(torch.isfinite(d["table"][~unpaired]).all())
    staged = int(bg.last_positions(f["plan"], bg.STACK_TILE).max()) + 1  # n_used of the stack's tile
    in_list = next(bt for bt in f["plan"]["batches"] if bg.STACK_TILE in bt["tiles"].tolist())
    ids = in_list["ids"][in_list["tiles"].tolist().index(bg.STACK_TILE), :staged]
    print(f"nan-colours: {int(unpaired.sum())} NaN rows, {int(unpaired[ids].sum())} of them among the {staged} records pass 2 stages")
    consistent(dev, key, 3, "nan")
    v_g2d, v_colors = backward(dev, key, 3, "nan")
    assert bool(torch.isfinite(v_g2d).all()) and bool(torch.isfinite(v_colors).all())
    assert not v_g2d[unpaired].any() and not v_colors[unpaired].any()
    check(compare("nan-colours", (v_g2d, v_colors), d))


def _nan_split(pl, nan_rows):
    """For a table whose rows `nan_rows` are NaN: (clean bool [N], exposed).  A pixel is dirty when a NaN row has a valid pair at it:
    its render is NaN, and so is, rightly, everything the kernel adds from it.  clean = the Gaussians with valid pairs at clean pixels
    only, whose rows must not notice.  exposed = how often the kernel's selects are what keeps them from it: (wave, record) pairs in
    which a clean Gaussian's record is valid at one lane while another lane of the same wave (64 pixels: 4 rows of the tile) already
    carries a NaN-coloured record from behind it in its accumulated colour."""
    touched = torch.zeros(pl["n"], dtype=torch.bool)
    hits = []
    for bt in pl["batches"]:
        hit = bt["mask"] & nan_rows[bt["ids"]][:, None, :]
        hits.append(hit)
        touched[bt["ids"][(bt["mask"] & hit.any(dim=2)[:, :, None]).any(dim=1)]] = True
    clean = pl["paired"] & ~touched & ~nan_rows
    exposed = 0
    for bt, hit in zip(pl["batches"], hits):
        behind = (hit.flip(2).cumsum(dim=2).flip(2) - hit.long()) > 0  # a NaN-coloured valid record at a later list position
        valid = bt["mask"] & clean[bt["ids"]][:, None, :]
        B, _, L = hit.shape
        exposed += int((valid.reshape(B, 4, 64, L).any(dim=2) & behind.reshape(B, 4, 64, L).any(dim=2)).sum())
    return clean, exposed


def test_non_finite_colours_of_valid_pairs_stay_at_their_pixels(dev):
    """The select-not-multiply rule where it decides something.  (The Gaussians of the test above contribute nowhere, and a record no
    lane of a wave takes is skipped before its colour is read.)  Here every 16th Gaussian of T0 has a NaN colour AND valid pairs: the
    pixels that take one are NaN, rightly; the Gaussians whose pairs all lie at other pixels must come out finite and within the rule
    of the reference run with zeros in those rows -- although they share waves with lanes whose accumulated colour is NaN."""
    f, d = front(dev, T0), data(dev, T0, 3)
    pl = f["plan"]
    nan_rows = pl["paired"] & (torch.arange(f["n"]) % 16 == 0)
    clean, exposed = _nan_split(pl, nan_rows)
    print(f"nan-valid: {int(nan_rows.sum())} NaN rows, {int(clean.sum())} clean Gaussians, {exposed} exposed (wave, record) pairs")
    assert int(nan_rows.sum()) >= 20 and int(clean.sum()) >= 40 and exposed >= 20
    table = torch.where(nan_rows[:, None], torch.full_like(d["colors"], float("nan")), d["colors"])
    # (at a clean pixel no NaN row is valid: what it adds does not read those colours, so the seeded reference is the truth there)
    v_colors, v_g2d = f["eng"].render_pixels_backward(f["view"], table.to(dev), d["v_out"].to(dev), d["v_alpha"].to(dev))
    v_g2d, v_colors = v_g2d.cpu(), v_colors.cpu()
    assert bool(torch.isnan(v_g2d[nan_rows]).any())  # the NaN did reach the rows it belongs to (v_colors reads no colour)
    assert bool(torch.isfinite(v_g2d[clean]).all()) and bool(torch.isfinite(v_colors[clean]).all())
    rows_of = {k: dict(v_g2d=d[k]["v_g2d"][clean], v_colors=d[k]["v_colors"][clean]) for k in ("truth", "floor")}
    check(compare("nan-valid", (v_g2d[clean], v_colors[clean]), rows_of))
