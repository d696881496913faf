"""No-GPU checks of the depth losses: the numpy float32 restatement (tests/depth_loss_ref.py) against the reference
trainer's lines written literally in torch and evaluated in float64; csrc/depth_math.h compiled for the host -- plainly and under
-fsanitize=address,undefined, a stand-alone program both times -- giving the restatement's bytes; the mutants the comparison must
catch; scene_io.view_depth_points on a committed COLMAP model; the C ABI's argument checks; header, map and _lib in agreement; the
command line's namespace; what depth.py and the train_scene keywords refuse without a device.
"""
import argparse
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import depth_loss_ref as ref
import gsbp_amd
from gsbp_amd import _lib, scene_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
H, W, CH = 13, 19, 3
NAMES = ("gwbp_depth_points_loss", "gwbp_depth_points_backward", "gwbp_depth_map_loss", "gwbp_depth_map_backward")


@pytest.fixture(scope="module")
def case():
    render, alpha = ref.make_image(H, W, 4, CH)
    points, g = ref.make_points(4 * _lib.DEPTH_BLOCK + 3, H, W)
    gmap, wmap = ref.make_depth_map(H, W)
    return dict(A=render[..., CH].copy(), render=render, alpha=alpha, points=points, g=g, gmap=gmap, wmap=wmap)


@pytest.fixture(scope="module")
def host_programs(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (c++, g++, clang++) found")
    d = tmp_path_factory.mktemp("depth_host")
    base = [cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"]
    src = os.path.join(ROOT, "tests", "depth_host.cpp")
    plain, checked = str(d / "depth_host"), str(d / "depth_host_san")
    subprocess.check_call(base + ["-O2", "-o", plain, src])
    subprocess.check_call(base + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", checked, src])
    return plain, checked, d


def run_host(exe, tmp, c, kind, c_points, c_map):
    src, dst = os.path.join(str(tmp), "depth_in.bin"), os.path.join(str(tmp), "depth_out.bin")
    M = c["points"].shape[0]
    with open(src, "wb") as f:
        f.write(struct.pack("<iiiiff", H, W, M, _lib.DEPTH_KINDS[kind], c_points, c_map))
        for k in ("A", "alpha", "points", "g", "gmap", "wmap"):
            f.write(np.ascontiguousarray(c[k], F).tobytes())
    subprocess.check_call([exe, src, dst])
    raw = open(dst, "rb").read()
    assert len(raw) == 4 * (10 * M + 3 * H * W)
    a = np.frombuffer(raw, F)
    per_point, per_pixel = a[:10 * M].reshape(M, 10), a[10 * M:].reshape(H, W, 3)
    return dict(d=per_point[:, 0], t=per_point[:, 1], v_A=per_point[:, 2:6], v_a=per_point[:, 6:10], map_t=per_pixel[..., 0],
                map_v_A=per_pixel[..., 1], map_v_a=per_pixel[..., 2]), raw


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, F).view(np.uint32), np.ascontiguousarray(b, F).view(np.uint32))


# ---- the point sets keep their promises ---------------------------------------------------------------------------------------------
def test_the_cases_hold_what_the_tests_need(case):
    pts, g, alpha = case["points"], case["g"], case["alpha"]
    t = ref.point_terms32(case["A"], alpha, pts, g)
    assert (pts[0] == 0).all() and ((pts == np.floor(pts)).all(axis=1)).sum() >= 4
    assert ((pts[:, 0] > W - 1) & (pts[:, 0] < W)).any() and ((pts[:, 1] > H - 1) & (pts[:, 1] < H)).any()
    assert (pts[:, 0] >= 0).all() and (pts[:, 0] < W).all() and (pts[:, 1] >= 0).all() and (pts[:, 1] < H).all()
    cell = (np.floor(pts[:, 0]) == 8) & (np.floor(pts[:, 1]) == 6)
    assert cell.sum() >= 8
    touched = alpha[t["row"][t["inside"]], t["col"][t["inside"]]]
    assert (touched == 0).any() and ((touched > 0) & (touched < ref.AMIN)).any() and (touched == 1).any()
    assert (t["d"] == 0).any() and (t["d"] == 0).mean() <= 0.10       # empty samples exist and are few
    assert not t["inside"].all() and np.log10(g.max() / g.min()) > 5.0
    assert np.isfinite(t["t"]).all() and np.isfinite(t["v_A"]).all() and np.isfinite(t["v_a"]).all()
    gm, wm = case["gmap"], case["wmap"]
    assert (gm == 0).any() and (gm < 0).any() and (wm == 0).any() and ((gm > 0) & (wm > 0)).sum() > H * W // 3


# ---- restatement against the literal torch statement ----------------------------------------------------------------------------------
def test_the_restatement_agrees_with_the_literal_statement_in_float64(case):
    """grid_sample normalises x to x / (W - 1) * 2 - 1 and back: a few float64 roundings of the coordinate; agreement to 1e-12."""
    A, alpha, pts, g = case["A"], case["alpha"], case["points"], case["g"]
    t64 = ref.point_terms64(A, alpha, pts, g)
    lit_loss, lit_d = ref.literal_point_loss(torch.from_numpy(case["render"]).double(), torch.from_numpy(alpha).double(),
                                             torch.from_numpy(pts).double(), torch.from_numpy(g).double(), channel=CH, scale=1.7)
    assert torch.isfinite(lit_loss) and np.isfinite(lit_d.numpy()).all()
    np.testing.assert_allclose(t64["d"], lit_d.numpy(), rtol=1e-12, atol=1e-13)
    want = np.float64(1.7) * np.sum(t64["t"]) / len(g)
    assert abs(float(lit_loss) - want) <= 1e-12 * abs(want)
    # the convention, pinned: column j is sampled at x = j, and beyond the last column the padding is ZERO, not the edge
    e = (A.astype(np.float64) / np.maximum(alpha.astype(np.float64), np.float64(ref.AMIN)))
    probe = np.array([[4.0, 6.0], [W - 1.0, 5.0], [W - 0.5, 5.0], [3.0, H - 0.25]], F)
    d = ref.point_terms64(A, alpha, probe, np.ones(4, F))["d"]
    _, lit = ref.literal_point_loss(torch.from_numpy(case["render"]).double(), torch.from_numpy(alpha).double(),
                                    torch.from_numpy(probe).double(), torch.ones(4).double(), channel=CH)
    np.testing.assert_allclose(d, [e[6, 4], e[5, W - 1], 0.5 * e[5, W - 1], 0.25 * e[H - 1, 3]], rtol=1e-15)
    np.testing.assert_allclose(lit.numpy(), d, rtol=1e-12)


def test_the_gradient_of_the_restatement_is_the_literal_statements_where_that_is_finite(case):
    A, alpha, g = case["A"], case["alpha"], case["g"]
    t32 = ref.point_terms32(A, alpha, case["points"], g)
    keep = t32["d"] > 0                                        # torch is NaN for the others: the stated departure
    pts, g = case["points"][keep], g[keep]
    M = len(g)
    render = torch.from_numpy(case["render"]).double().requires_grad_(True)
    a = torch.from_numpy(alpha).double().requires_grad_(True)
    loss, _ = ref.literal_point_loss(render, a, torch.from_numpy(pts).double(), torch.from_numpy(g).double(), channel=CH, scale=2.0)
    loss.backward()
    t64 = ref.point_terms64(A, alpha, pts, g, c=2.0 / M)
    vA, va, absA, absa, _, _ = ref.scatter_maps(t64, H, W)
    assert torch.isfinite(render.grad).all() and torch.isfinite(a.grad).all()
    np.testing.assert_allclose(render.grad[..., CH].numpy(), vA, rtol=0, atol=1e-11 * absA.max())
    np.testing.assert_allclose(a.grad.numpy(), va, rtol=0, atol=1e-11 * absa.max())
    assert not render.grad[..., :CH].any()
    # with the empty samples the literal statement is NaN, the restatement finite: zeros from those points
    render.grad = a.grad = None
    loss, _ = ref.literal_point_loss(render, a, torch.from_numpy(case["points"]).double(), torch.from_numpy(case["g"]).double(), channel=CH)
    loss.backward()
    assert torch.isnan(render.grad).any()
    empty = ref.point_terms32(A, alpha, case["points"][~keep], case["g"][~keep])
    assert not empty["v_A"].any() and not empty["v_a"].any() and same_bits(empty["t"], F(1) / case["g"][~keep])


def test_float32_restatement_stays_within_the_bound_of_the_truth(case):
    A, alpha, pts, g = case["A"], case["alpha"], case["points"], case["g"]
    c = ref.scale_over_m(1.3, len(g))
    t32, t64 = ref.point_terms32(A, alpha, pts, g, c), ref.point_terms64(A, alpha, pts, g, c)
    m32, m64 = ref.scatter_maps(t32, H, W), ref.scatter_maps(t64, H, W)
    for k in (0, 1):
        assert (np.abs(m32[k] - m64[k]) <= ref.grad_bound(m64[4 + k], m64[2 + k])).all()


# ---- the header on the host -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["disparity", "depth"])
def test_the_header_on_the_host_gives_the_restatements_bytes(host_programs, case, kind):
    plain, checked, tmp = host_programs
    c_points = float(ref.scale_over_m(1.3, len(case["g"])))
    sw = ref.map_sums64(ref.map_terms32(case["A"], case["alpha"], case["gmap"], case["wmap"], kind))[1]
    c_map = float(ref.map_c(0.75, 1.3, sw))
    got, raw = run_host(plain, tmp, case, kind, c_points, c_map)
    want = ref.point_terms32(case["A"], case["alpha"], case["points"], case["g"], c_points)
    for k in ("d", "t", "v_A", "v_a"):
        assert same_bits(got[k], want[k]), k
    wmap = ref.map_terms32(case["A"], case["alpha"], case["gmap"], case["wmap"], kind, c_map)
    for k in ("t", "v_A", "v_a"):
        assert same_bits(got["map_" + k], wmap[k]), k
    assert wmap["v_A"].any() and wmap["v_a"].any() and want["v_A"].any() and want["v_a"].any()
    # the same text under the address and undefined-behaviour sanitizers: a clean run and the same bytes
    assert run_host(checked, tmp, case, kind, c_points, c_map)[1] == raw


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_the_comparison_catches_the_mutants(host_programs, case, mutant):
    plain, _, tmp = host_programs
    c_points = float(ref.scale_over_m(1.3, len(case["g"])))
    got, _ = run_host(plain, tmp, case, "disparity", c_points, 1.0)
    bad = ref.point_terms32(case["A"], case["alpha"], case["points"], case["g"], c_points, mutant=mutant)
    differs = {k: not same_bits(got[k], bad[k]) for k in ("d", "t", "v_A", "v_a")}
    print(mutant, differs)
    expect = {"pixel_centre": ("d", "t", "v_A", "v_a"), "clamped_padding": ("d", "t", "v_A"), "eps_division": ("t", "v_A"),
              "no_q2": ("v_A", "v_a"), "no_alpha_rule": ("v_a",)}[mutant]
    assert all(differs[k] for k in expect), differs
    # ... and by far more than rounding: against the float64 truth the mutant's maps leave the bound
    t64 = ref.point_terms64(case["A"], case["alpha"], case["points"], case["g"], c_points)
    m64, mbad = ref.scatter_maps(t64, H, W), ref.scatter_maps(bad, H, W)
    worst = max(float(np.nanmax(np.where(np.abs(mbad[k] - m64[k]) > ref.grad_bound(m64[4 + k], m64[2 + k]), 1.0, 0.0))) for k in (0, 1))
    assert worst == 1.0 or not np.isfinite(mbad[0]).all() or not np.isfinite(mbad[1]).all()


# ---- the view's points ----------------------------------------------------------------------------------------------------------------
def test_view_depth_points_against_a_float64_projection_of_the_tracks():
    proj = scene_io.read_colmap_model(os.path.join(ROOT, "tests", "golden", "colmap_depth", "sparse", "0"))
    cam = next(iter(proj.cameras.values()))
    K = scene_io.camera_matrix(cam)
    Wd, Hd = cam.width, cam.height
    reasons = set()
    for iid, im in proj.images.items():
        want_xy, want_z = [], []
        vm = scene_io.get_viewmat_from_colmap_image(im).double().numpy()
        vm[:3, :3], vm[:3, 3] = im.R(), im.tvec  # (float64 throughout)
        for pid, xyz in zip(proj.point3D_ids, proj.points3D):
            for track_image, _ in proj.point3D_id_to_images[int(pid)]:
                if track_image != iid:
                    continue
                p = vm[:3, :3] @ xyz + vm[:3, 3]
                x, y = cam.fx * p[0] / p[2] + cam.cx, cam.fy * p[1] / p[2] + cam.cy
                drop = [name for name, hit in (("left", x < 0), ("right", x >= Wd), ("above", y < 0), ("below", y >= Hd),
                                               ("behind", p[2] <= 0)) if hit]
                reasons.update(drop if iid == 1 else [])
                if not drop:
                    want_xy.append((x, y)), want_z.append(p[2])
        pts, depths = scene_io.view_depth_points(proj, im, K, Wd, Hd)
        assert pts.dtype == torch.float32 and depths.dtype == torch.float32 and not pts.is_cuda
        assert tuple(pts.shape) == (len(want_z), 2) and tuple(depths.shape) == (len(want_z),)
        np.testing.assert_allclose(pts.numpy(), np.array(want_xy).reshape(-1, 2), rtol=2.0 ** -23)
        np.testing.assert_allclose(depths.numpy(), np.array(want_z), rtol=2.0 ** -23)
        same = scene_io.view_depth_points(proj, iid, K, Wd, Hd)
        assert torch.equal(same[0], pts) and torch.equal(same[1], depths)
    assert reasons == {"left", "right", "above", "below", "behind"}
    pts, depths = scene_io.view_depth_points(proj, 1, K, Wd, Hd)
    assert len(depths) == 5 and depths.tolist() == [4.0, 5.0, 4.0, 6.0, 6.0]  # 101, 102, 103 and 109 twice
    assert pts[0].tolist() == [32.0, 24.0] and pts[2].tolist() == [0.75, 46.75]


# ---- the C ABI: nothing here reaches a kernel ------------------------------------------------------------------------------------------
def test_header_map_and_lib_agree():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gwbp.h")).read(), flags=re.S)
    text = open(os.path.join(ROOT, "3dgs-gradient-backprojection_amd", "csrc", "gwbp.map")).read()
    gsbp_amd.build()
    for name in NAMES:
        proto = re.search(r"GWBP_API int " + name + r"\s*\(([^;]*)\)\s*;", src)
        assert proto, name
        assert len(proto.group(1).split(",")) == len(_lib.ARGTYPES[name]), name
        assert name in _lib.EXPORTS and name in text and hasattr(_lib.lib(), name)
    assert "gwbp_*" in text
    assert "depth_loss.hip" in open(os.path.join(ROOT, "3dgs-gradient-backprojection_amd", "csrc", "Makefile")).read()
    assert re.search(r"#define GWBP_DEPTH_BLOCK\s+%d\b" % _lib.DEPTH_BLOCK, src)
    for kind, code in _lib.DEPTH_KINDS.items():
        assert re.search(r"#define GWBP_DEPTH_KIND_%s\s+%d\b" % (kind.upper(), code), src)
    assert _lib.depth_workspace_bytes(0) == 0 and _lib.depth_workspace_bytes(1) == 16 and _lib.depth_workspace_bytes(257) == 32
    for fn in ("depth_points_loss", "depth_points_backward", "depth_map_loss", "depth_map_backward"):
        assert callable(getattr(gsbp_amd.Engine, fn))
    assert callable(gsbp_amd.depth_point_loss) and callable(gsbp_amd.depth_map_loss)


def test_capi_rejects_without_a_launch():
    lib = _lib.lib()
    buf = (C.c_float * 16384)()
    a = (C.addressof(buf) + 15) & ~15

    def message():
        return lib.gwbp_last_error_string().decode()

    def at(i):
        return a + 4096 * i

    def points_loss(H=4, W=4, Dp=4, ch=3, render=at(0), alpha=at(1), M=5, points=at(2), depths=at(3), loss=at(4), per_point=None,
                    ws=at(5), ws_bytes=4096):
        return lib.gwbp_depth_points_loss(H, W, Dp, ch, render, alpha, M, points, depths, 1.0, loss, per_point, ws, ws_bytes, None)

    def points_backward(H=4, W=4, Dp=4, ch=3, render=at(0), alpha=at(1), M=5, points=at(2), depths=at(3), upstream=at(4),
                        v_render=at(5), v_alpha=at(6)):
        return lib.gwbp_depth_points_backward(H, W, Dp, ch, render, alpha, M, points, depths, 1.0, upstream, v_render, v_alpha, None)

    def map_loss(H=4, W=4, Dp=4, ch=3, render=at(0), alpha=at(1), depth=at(2), weights=None, kind=0, loss=at(4), sums=at(6),
                 ws=at(5), ws_bytes=4096):
        return lib.gwbp_depth_map_loss(H, W, Dp, ch, render, alpha, depth, weights, kind, 1.0, loss, sums, ws, ws_bytes, None)

    def map_backward(H=4, W=4, Dp=4, ch=3, render=at(0), alpha=at(1), depth=at(2), weights=None, kind=0, sums=at(6), upstream=at(4),
                     v_render=at(5), v_alpha=at(7)):
        return lib.gwbp_depth_map_backward(H, W, Dp, ch, render, alpha, depth, weights, kind, 1.0, sums, upstream, v_render, v_alpha,
                                           None)

    for call in (points_loss, points_backward, map_loss, map_backward):
        for bad in (dict(H=0), dict(W=0), dict(H=-3), dict(W=(1 << 24) + 1), dict(H=1 << 16, W=1 << 15), dict(H=1 << 24, W=1 << 24)):
            assert call(**bad) == -1 and "pixels" in message(), (call.__name__, bad)
        for bad in (dict(Dp=0), dict(ch=-1), dict(ch=4), dict(Dp=1, ch=1)):
            assert call(**bad) == -1 and "channel" in message(), (call.__name__, bad)
        for null in ("render", "alpha"):
            assert call(**{null: None}) == -1 and "null" in message(), (call.__name__, null)
        assert call(render=at(0) + 2) == -1 and "aligned" in message()
    for call in (points_loss, points_backward):
        for M in (-1, 1 << 31):
            assert call(M=M) == -1 and "points" in message()
        for null in ("points", "depths"):
            assert call(**{null: None}) == -1 and "null" in message()
    for call in (map_loss, map_backward):
        for kind in (-1, 2, 7):
            assert call(kind=kind) == -1 and "kind" in message()
        assert call(depth=None) == -1 and "null" in message()
    assert points_loss(loss=None) == -1 and "loss" in message()
    assert points_loss(ws=None) == -1 and "workspace" in message()
    assert points_loss(ws=at(5) + 4) == -1 and "workspace" in message()
    assert points_loss(M=257, ws_bytes=16) == -2 and "needs 32" in message()
    assert map_loss(sums=None) == -1 and "sums" in message()
    assert map_loss(sums=at(6) + 4) == -1 and "sums" in message()
    assert map_loss(H=64, W=64, ws_bytes=16) == -2 and "workspace" in message()
    for call in (points_backward, map_backward):
        for null in ("upstream", "v_render", "v_alpha"):
            assert call(**{null: None}) == -1 and "null" in message(), (call.__name__, null)
        assert call(v_render=at(0)) == -1 and "input" in message()   # the gradient is the render
        assert call(v_alpha=at(5)) == -1 and "same array" in message()
    assert map_backward(sums=None) == -1 and "sums" in message()
    # nothing to do: no points, no launch, no device
    assert points_backward(M=0, points=None, depths=None) == 0
    del buf


# ---- the command line and the Python layer without a device ---------------------------------------------------------------------------
def test_the_command_lines_namespace_is_unchanged_without_the_options():
    import run_train
    ap = run_train.build_parser()
    plain = vars(ap.parse_args(["--synthetic", "T0"]))
    names = ("depth_loss", "depth_lambda", "depth_kind")
    assert not any(k in plain for k in names)
    for action in ap._actions:
        if action.dest in names:
            assert action.default is argparse.SUPPRESS
    given = vars(ap.parse_args(["--synthetic", "T0", "--depth-loss", "--depth-lambda", "0.5", "--depth-kind", "depth"]))
    assert given["depth_loss"] is True and given["depth_lambda"] == 0.5 and given["depth_kind"] == "depth"
    assert {k: v for k, v in given.items() if k not in names} == plain
    with pytest.raises(SystemExit):
        ap.parse_args(["--synthetic", "T0", "--depth-loss", "--depth-kind", "inverse"])
    with pytest.raises(SystemExit):
        run_train.main(["--synthetic", "T0", "--depth-lambda", "0.5"])  # needs --depth-loss


def test_depth_py_and_the_keywords_refuse_without_a_device():
    render, alpha = torch.zeros(5, 7, 4), torch.zeros(5, 7)
    pts, g = torch.zeros(3, 2), torch.ones(3)
    with pytest.raises(gsbp_amd.GwbpError, match="no CPU path"):
        gsbp_amd.depth_point_loss(render, alpha, pts, g)
    with pytest.raises(gsbp_amd.GwbpError, match="no CPU path"):
        gsbp_amd.depth_map_loss(render, alpha, torch.ones(5, 7))
    with pytest.raises(gsbp_amd.GwbpError, match="no CPU path"):
        gsbp_amd.sample_expected_depth(render, alpha, pts)
    with pytest.raises(gsbp_amd.GwbpError, match="no CPU path"):
        gsbp_amd.depth_point_loss(render.numpy(), alpha, pts, g)
    from gsbp_amd.engine import depth_image_args, depth_map_args, depth_point_args

    class Fake(torch.Tensor):  # a CPU tensor that says it is on the device: the checks behind the first one, without a device
        is_cuda = True

    def fake(*shape, dtype=torch.float32):
        return torch.zeros(*shape, dtype=dtype).as_subclass(Fake)

    for bad_render in (fake(5, 7), fake(5, 7, 4, dtype=torch.float64), fake(5, 7, 4, dtype=torch.float16), fake(0, 7, 4)):
        with pytest.raises(gsbp_amd.GwbpError, match="render must be"):
            depth_image_args("depth_point_loss", bad_render, fake(5, 7), -1)
    for bad_alpha in (fake(5, 6), fake(7, 5), fake(5, 7, 2)):
        with pytest.raises(gsbp_amd.GwbpError, match="alpha must be"):
            depth_image_args("depth_point_loss", fake(5, 7, 4), bad_alpha, -1)
    with pytest.raises(gsbp_amd.GwbpError, match="alpha must be float32"):
        depth_image_args("depth_point_loss", fake(5, 7, 4), fake(5, 7, dtype=torch.float64), -1)
    for channel in (4, -5, 1.0, True, None):
        with pytest.raises(gsbp_amd.GwbpError, match="channel"):
            depth_image_args("depth_point_loss", fake(5, 7, 4), fake(5, 7, 1), channel)
    assert depth_image_args("depth_point_loss", fake(5, 7, 4), fake(5, 7, 1), -1)[2:] == (5, 7, 4, 3)
    for p, d in ((fake(3, 3), fake(3)), (fake(3, 2), fake(4)), (fake(6), fake(3)), (fake(3, 2, dtype=torch.float64), fake(3))):
        with pytest.raises(gsbp_amd.GwbpError, match="points"):
            depth_point_args("depth_point_loss", fake(5, 7, 4), p, d)
    with pytest.raises(gsbp_amd.GwbpError, match="kind must be"):
        depth_map_args("depth_map_loss", fake(5, 7, 4), fake(5, 7), None, "inverse")
    for m, w in ((fake(5, 6), None), (fake(5, 7), fake(7, 5)), (fake(5, 7, dtype=torch.float16), None)):
        with pytest.raises(gsbp_amd.GwbpError, match="must be float32"):
            depth_map_args("depth_map_loss", fake(5, 7, 4), m, w, "depth")
    # train_scene: the keywords are checked before anything touches a device
    sc = gsbp_amd.synthetic.make_scene(gsbp_amd.synthetic.CONFIGS["T0"])
    sc["features_dc"], sc["features_rest"] = torch.zeros(512, 1, 3), torch.zeros(512, 15, 3)
    eye, K = torch.eye(4)[None], torch.eye(3)

    def train(**kw):
        return gsbp_amd.train_scene(sc, eye, K, 96, 64, lambda v: None, 10, **kw)

    with pytest.raises(gsbp_amd.GwbpError, match="render_mode"):
        train(depth_fn=lambda v: None, render_mode="RGB+ED")
    with pytest.raises(gsbp_amd.GwbpError, match="depth_fn must be"):
        train(depth_fn=(pts, g))
    with pytest.raises(gsbp_amd.GwbpError, match="depth_kind"):
        train(depth_fn=lambda v: None, depth_kind="inverse")
    for name in ("depth_lambda", "depth_scale"):
        for bad in (float("nan"), float("inf"), "1", True, None):
            with pytest.raises(gsbp_amd.GwbpError, match=name):
                train(depth_fn=lambda v: None, **{name: bad})
    with pytest.raises(gsbp_amd.GwbpError, match="no CPU path"):  # good keywords go on to the next check: the tensors' device
        train(depth_fn=lambda v: None, depth_lambda=0.5, depth_scale=2.0, depth_kind="depth")
    import inspect
    sig = inspect.signature(gsbp_amd.train_scene).parameters
    assert sig["depth_fn"].default is None and sig["depth_lambda"].default == 1e-2 and sig["depth_scale"].default == 1.0
    assert sig["depth_kind"].default == "disparity"
    assert inspect.signature(gsbp_amd.polish.render_splats).parameters["return_alpha"].default is False


def test_check_depth_options_alone():
    """depth.check_depth_options, the check train_scene makes: {} without a depth_fn whatever the other values are, the render's
    keywords with one, and for each bad value the text the test above expects from train_scene."""
    from gsbp_amd.depth import DEPTH_KINDS, check_depth_options

    def fn(v):
        return None
    for other in ((1e-2, 1.0, "disparity", {}), (float("nan"), None, "inverse", dict(render_mode="RGB+ED")), ("1", True, 7, dict(eps2d=0.3))):
        assert check_depth_options("train_scene", None, *other) == {}
    assert check_depth_options("train_scene", fn, 0.5, 2, "depth", dict(eps2d=0.3)) == dict(render_mode="RGB+D", return_alpha=True)
    assert DEPTH_KINDS == tuple(_lib.DEPTH_KINDS) == ("disparity", "depth")
    with pytest.raises(gsbp_amd.GwbpError, match=r"train_scene\(depth_fn=\.\.\.\) renders with render_mode='RGB\+D'"):
        check_depth_options("train_scene", fn, 1e-2, 1.0, "disparity", dict(render_mode="RGB+ED"))
    with pytest.raises(gsbp_amd.GwbpError, match=r"train_scene\(\): depth_fn must be a callable of the view's index, got tuple"):
        check_depth_options("train_scene", (1, 2), 1e-2, 1.0, "disparity", {})
    with pytest.raises(gsbp_amd.GwbpError, match=r"train_scene\(\): depth_kind must be one of \['disparity', 'depth'\], got 'inverse'"):
        check_depth_options("train_scene", fn, 1e-2, 1.0, "inverse", {})
    for name in ("depth_lambda", "depth_scale"):
        for bad in (float("nan"), float("inf"), "1", True, None):
            values = dict(dict(depth_lambda=1e-2, depth_scale=1.0), **{name: bad})
            with pytest.raises(gsbp_amd.GwbpError, match=rf"my_loop\(\): {name} must be a finite number, got "):
                check_depth_options("my_loop", fn, values["depth_lambda"], values["depth_scale"], "disparity", {})
