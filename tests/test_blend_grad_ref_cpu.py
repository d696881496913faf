"""No-GPU checks of the list-based yardstick of the blend backward (tests/blend_grad_ref.py): lists and pairs from the CPU oracle.

    (a) in float64 it IS the dense yardstick's blend (tests/raster_grad_ref.py) on the same cut: render, alpha map, colour gradient
    (b) its gradients equal central finite differences of its own loss, the mask held fixed
    (c) the comparison rule of tests/test_gpu_blend_grad.py has teeth at the factor chosen there: a dropped record, a doubled cb
        column, a ca column without its 1/2 and a missing v_alpha term all FAIL it
    (d) the scenes of the GPU test sit where they are meant to sit (list lengths, termination on both sides of the first batch)
"""
import functools

import pytest
import torch

import blend_grad_ref as bg
import raster_grad_ref as rg
from gsbp_amd.projection import project_torch
from test_gpu_blend_grad import FACTOR, LIST_LENGTHS
from test_gpu_raster_grad import _stack, _t0


def _scene(name):
    if name == "t0":
        return _t0()
    return _stack(0.1, n=80)


@functools.lru_cache(maxsize=None)
def _case(name, orc):
    """The scene, the oracle's front and cut, seeded v_out / v_alpha; computed once, never modified."""
    sc = _scene(name)
    f = bg.oracle_front(orc, *sc["inputs"][:4], sc["vm"], sc["K"], sc["W"], sc["H"])
    g = torch.Generator().manual_seed(41)
    return dict(sc=sc, front=f, colors=sc["inputs"][4], v_out=torch.randn(sc["H"], sc["W"], 3, generator=g),
                v_alpha=torch.randn(sc["H"], sc["W"], generator=g))


@pytest.mark.parametrize("name", ["t0", "stack80"])
def test_float64_equals_the_dense_yardstick_on_the_same_cut(orc, name):
    """Both sides read project_torch's float64 records (the dense yardstick projects for itself), the oracle's lists and pairs."""
    c = _case(name, orc)
    sc, f = c["sc"], c["front"]
    W, H = sc["W"], sc["H"]
    n = sc["inputs"][0].shape[0]
    visible = torch.from_numpy(f["proj"]["radii"] > 0)
    cut = dict(mask=rg.pairs_mask(f["gid"], f["pix"], W * H, n), visible=visible,
               order=rg.depth_order(torch.from_numpy(f["proj"]["depths"]), visible))
    assert int(cut["mask"].sum()) == len(f["gid"]) > 2000
    ins = [t.double() for t in sc["inputs"]]
    m2d, con, oe = project_torch(*ins[:4], sc["vm"], sc["K"], W, H, 0.3, "pinhole", "classic", visible)
    got = bg.blend(torch.float64, f["plan"], m2d, con, oe, ins[4], c["v_out"], c["v_alpha"])
    out, alpha, _ = rg.render(*ins, sc["vm"], sc["K"], W, H, cut)
    grads, loss, _ = rg.gradients(torch.float64, sc["inputs"], c["v_out"], c["v_alpha"], sc["vm"], sc["K"], W, H, cut)
    figs = dict(out=rg.errors(got["out"], out), alpha=rg.errors(got["alpha_img"], alpha), v_colors=rg.errors(got["v_colors"], grads[4]),
                loss=abs(float(got["loss"] - loss)) / abs(float(loss)))
    print(name, figs)
    assert float(out.abs().max()) > 0.1 and float(grads[4].abs().max()) > 0
    assert max(figs["out"]) <= 1e-12 and max(figs["alpha"]) <= 1e-12 and max(figs["v_colors"]) <= 1e-12 and figs["loss"] <= 1e-12


@pytest.mark.parametrize("name", ["t0", "stack80"])
def test_gradients_equal_finite_differences_of_the_reference_own_loss(orc, name):
    """20 seeded record entries, spread over the six columns, among the Gaussians that have a valid pair; the mask is the plan's:
    held fixed.  Central differences in float64 at a step of 1e-5 of the entry's size: ~1e-10 truncation, ~1e-8 rounding."""
    c = _case(name, orc)
    f = c["front"]
    rec = [f["means2d"].double(), f["conics"].double(), f["opacities"].double()]
    truth = bg.blend(torch.float64, f["plan"], *rec, c["colors"], c["v_out"], c["v_alpha"])
    paired = torch.nonzero(f["plan"]["paired"]).reshape(-1)
    g = torch.Generator().manual_seed(43)
    picks = [(int(paired[int(torch.randint(len(paired), (1,), generator=g))]), k % 6) for k in range(20)]

    def loss_at(row, col, delta):
        r = [t.clone() for t in rec]
        t, j = (r[0], col) if col < 2 else (r[1], col - 2) if col < 5 else (r[2], None)
        if j is None:
            t[row] += delta
        else:
            t[row, j] += delta
        return float(bg.blend(torch.float64, f["plan"], *r, c["colors"], c["v_out"], c["v_alpha"], grads=False)["loss"])

    fd, ag = torch.zeros(20, dtype=torch.float64), torch.zeros(20, dtype=torch.float64)
    for i, (row, col) in enumerate(picks):
        x = float(torch.cat([rec[0], rec[1], rec[2][:, None]], dim=1)[row, col])
        h = 1e-5 * max(abs(x), 1e-2)
        fd[i] = (loss_at(row, col, h) - loss_at(row, col, -h)) / (2 * h)
        ag[i] = truth["v_g2d"][row, col]
    assert sorted(set(col for _, col in picks)) == list(range(6))
    for col in range(6):  # (per column: the six differ in scale by orders of magnitude)
        sel = torch.tensor([i for i, p in enumerate(picks) if p[1] == col])
        fro, top = rg.errors(ag[sel], fd[sel])
        print(f"{name} {bg.COLUMNS[col]}: autograd against central differences: {fro:.2e} (Frobenius), {top:.2e} (max)")
        assert float(fd[sel].abs().max()) > 0 and fro < 1e-6 and top < 1e-6, bg.COLUMNS[col]


@functools.lru_cache(maxsize=None)
def _teeth(orc):
    """The stack of 600 at opacity 0.02 (nobody terminates: the record at list position 256 counts at most of the tile's pixels):
    truth, floor and plan."""
    sc = _stack(0.02)
    f = bg.oracle_front(orc, *sc["inputs"][:4], sc["vm"], sc["K"], sc["W"], sc["H"])
    g = torch.Generator().manual_seed(47)
    args = (f["means2d"], f["conics"], f["opacities"], sc["inputs"][4], torch.randn(sc["H"], sc["W"], 3, generator=g),
            torch.randn(sc["H"], sc["W"], generator=g))
    return dict(front=f, args=args, truth=bg.blend(torch.float64, f["plan"], *args), floor=bg.blend(torch.float32, f["plan"], *args))


def test_the_float32_truth_passes_the_rule(orc):
    """The float64 gradients rounded to float32 are within the factor of the float32 run's error: the rule can be met."""
    t = _teeth(orc)
    rows = bg.report("rounded", (t["truth"]["v_g2d"].float(), t["truth"]["v_colors"].float()), t["truth"], t["floor"])
    bg.show(rows)
    assert len(rows) == 18 and all(r["floor"] > 0 for r in rows)
    assert not bg.failures(rows, FACTOR)


@pytest.mark.parametrize("what", ["dropped-record", "cb-doubled", "ca-without-half", "no-v_alpha"])
def test_doctored_outputs_fail_the_rule(orc, what):
    t = _teeth(orc)
    f, truth = t["front"], t["truth"]
    v_g2d, v_colors = truth["v_g2d"].float(), truth["v_colors"].float()
    if what == "dropped-record":
        assert bg.list_length(f["plan"], bg.STACK_TILE) == 600
        took = next(bt for bt in f["plan"]["batches"] if bg.STACK_TILE in bt["tiles"].tolist())
        assert int(took["mask"][took["tiles"].tolist().index(bg.STACK_TILE), :, 256].sum()) > 100  # (most pixels take it)
        less = bg.blend(torch.float64, f["plan"], *t["args"], skip=[(bg.STACK_TILE, 256)])
        v_g2d, v_colors = less["v_g2d"].float(), less["v_colors"].float()
        quantities = set(bg.QUANTITIES) | {"mean", "conic", "opacity"}
    elif what == "cb-doubled":
        v_g2d[:, 3] *= 2.0
        quantities = {"cb", "conic"}
    elif what == "ca-without-half":
        v_g2d[:, 2] *= 2.0
        quantities = {"ca", "conic"}
    else:
        less = bg.blend(torch.float64, f["plan"], *t["args"][:5], None)
        v_g2d, v_colors = less["v_g2d"].float(), less["v_colors"].float()
        quantities = set(bg.COLUMNS) | {"mean", "conic", "opacity"}  # (the colour gradient does not read v_alpha)
    rows = bg.report(what, (v_g2d, v_colors), truth, t["floor"])
    bad = bg.failures(rows, FACTOR)
    bg.show(bad)
    assert set(r["quantity"] for r in bad) == quantities, what
    # ... by orders of magnitude: no factor up to the ceiling the rule may ever take (16) lets one of them through
    assert set(r["quantity"] for r in bg.failures(rows, 16.0)) == quantities
    assert min(r["kernel"] / r["floor"] for r in bad) > 100.0


def test_without_colours_the_colour_figures_are_left_out(orc):
    t = _teeth(orc)
    rows = bg.report("no-colours", (t["truth"]["v_g2d"].float(), None), t["truth"], t["floor"])
    assert len(rows) == 15 and not any(r["quantity"] == "colors" for r in rows)


def test_all_zero_truth_takes_no_difference_at_all():
    z = torch.zeros(5, 3, dtype=torch.float64)
    assert bg.row_error(z.float(), z) == 0.0 and bg.row_error(z.float() + 1e-30, z) == 1.0


# ---- (d) the GPU test's scenes, on the oracle's cut -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", LIST_LENGTHS)
def test_list_length_scenes_have_that_length_and_nobody_terminates(orc, n):
    sc = _stack(0.02, n=n)
    f = bg.oracle_front(orc, *sc["inputs"][:4], sc["vm"], sc["K"], sc["W"], sc["H"])
    assert bg.list_length(f["plan"], bg.STACK_TILE) == n
    g = torch.Generator().manual_seed(n)
    ref = bg.blend(torch.float64, f["plan"], f["means2d"], f["conics"], f["opacities"], sc["inputs"][4],
                   torch.randn(sc["H"], sc["W"], 3, generator=g), grads=False)
    assert bg.nobody_terminates(ref, 0.02)
    assert int(bg.last_positions(f["plan"], bg.STACK_TILE).max()) == n - 1  # somebody takes the list's last record


@pytest.mark.parametrize("opacity", bg.TERMINATION_OPACITIES)
def test_termination_scenes_end_on_both_sides_of_the_first_batch(orc, opacity):
    sc = _stack(opacity)
    f = bg.oracle_front(orc, *sc["inputs"][:4], sc["vm"], sc["K"], sc["W"], sc["H"])
    lo, hi, kinds = bg.check_termination(f["plan"])
    print(f"opacity {opacity}: last positions {lo} .. {hi}, {kinds} different; {int((~f['plan']['paired']).sum())} Gaussians unpaired")
    assert int((~f["plan"]["paired"]).sum()) >= 1
    assert (hi - 1) // 256 == (2 if opacity == 0.15 else 1)
