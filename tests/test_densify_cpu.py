"""No-GPU checks of densification: the numpy yardstick against itself -- the fused rule against gsplat's literal two
steps, the mutants it must catch, the float32 split against float64 -- csrc/densify_math.h compiled for the host against the yardstick
bit for bit, the C ABI's argument checks, and what the Python layer refuses without a device.
"""
import ctypes as C
import math
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import densify_ref as ref
import gsbp_amd
from gsbp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 2000


# ---- the data: thresholds at the medians, so that every action and every prune reason occurs ----------------------------------------
def scene(n=N, seed=5, extra=8):
    r = np.random.default_rng(seed)
    t = dict(means=ref.f32(r.normal(size=(n, 3))), scaling=ref.f32(math.log(0.05) + 0.7 * r.normal(size=(n, 3))),
             rotation=ref.f32(r.normal(size=(n, 4))), opacity=ref.f32(2.0 * r.normal(size=n)), field=ref.f32(r.normal(size=(n, extra))))
    count = ref.f32(r.integers(0, 6, size=n))
    grad2d = ref.f32(np.abs(r.normal(size=n)) * 1e-3 * np.maximum(count, 1))
    noise = ref.f32(r.normal(size=(n, 2, 3)))
    m = ref.largest_scale(t["scaling"])
    g = grad2d / np.maximum(count, 1)
    # every threshold IS a value of the data (the median of an odd count): ties exist, so > against >= can be told apart
    odd = slice(0, n - 1 + n % 2)
    th = (float(np.median(g[odd])), float(np.median(m[odd])), float(np.median(m[odd])) + 0.3, float(np.quantile(t["opacity"], 0.2)),
          float(np.float32(math.log(1.6))))
    # ... and ten rows sit exactly on the gradient threshold with an opacity that keeps them
    grad2d[10:20], count[10:20], t["opacity"][10:20] = np.float32(th[0]), 1.0, 5.0
    return t, grad2d, count, noise, th


def fused(t, grad2d, count, noise, th, prune_big, mutant=None, moments=None):
    """The fused rule's new set: plan -> emit -> gather, with `mutant` applied where it belongs."""
    kind, offsets = ref.plan(grad2d, count, t["scaling"], t["opacity"], th, prune_big,
                             mutant if mutant in ("ge_grad", "prune_before_shrink", "inclusive") else None)
    if mutant == "inclusive":  # what a kernel would do with an inclusive scan: every row lands one parent too late
        return kind, offsets, None, None
    new = ref.emit(kind, offsets, t["means"], t["scaling"], t["rotation"], t["opacity"], noise, th[4])
    out = {k: new[k] for k in ("means", "scaling", "rotation", "opacity")}
    for k in t:
        if k not in out:
            out[k] = ref.gather(t[k], new["parent"])
    mom = None if moments is None else ref.gather(moments, new["parent"], new["child"], kind, "zero_new",
                                                  mutant if mutant == "zero_original" else None)
    return kind, offsets, out, mom


@pytest.mark.parametrize("prune_big", [False, True])
def test_the_fused_rule_yields_the_rows_of_the_literal_two_steps(prune_big):
    t, grad2d, count, noise, th = scene()
    moments = ref.f32(np.random.default_rng(9).normal(size=(N, 3))) + np.float32(10.0)  # (never zero: a zeroed row is recognisable)
    kind, offsets, out, mom = fused(t, grad2d, count, noise, th, prune_big, moments=moments)
    lit, lit_mom = ref.literal_two_steps(grad2d, count, t, th, prune_big, noise, moments=moments)
    assert int(offsets[-1]) == len(out["means"]) == len(lit["means"]) > 0
    assert ref.row_multiset(out) == ref.row_multiset(lit)
    assert ref.row_multiset(dict(out, mom=mom)) == ref.row_multiset(dict(lit, mom=lit_mom))
    # the eight combinations of the three tests are all hit, and so is every prune reason
    low, high, small, m = ref.flags(grad2d, count, t["scaling"], t["opacity"], th)
    seen = {(bool(a), bool(b), bool(c)) for a, b, c in zip(low, high, small)}
    assert len(seen) == 8
    assert {int(k) for k in kind} == {0, 1, 2, 3}
    if prune_big:
        big, child_big = m > np.float32(th[2]), (m - np.float32(th[4])) > np.float32(th[2])
        assert (~low & ~high & big).any() and (~low & high & ~small & child_big).any()  # a keep and a split leave for their size
        assert (~low & high & ~small & big & ~child_big).any()                           # a split whose children are small enough
    assert (low & high & small).any() and (low & high & ~small).any()                    # a clone and a split leave for their opacity
    assert (np.asarray(count) == 0).any()
    # offsets: exclusive, children adjacent, parent order
    rows = ref.ROWS_OUT[kind]
    assert offsets[0] == 0 and np.array_equal(np.diff(offsets), rows)


@pytest.mark.parametrize("mutant", ["prune_before_shrink", "ge_grad", "zero_original", "inclusive"])
def test_mutants_fail(mutant):
    t, grad2d, count, noise, th = scene()
    moments = ref.f32(np.random.default_rng(9).normal(size=(N, 3))) + np.float32(10.0)
    lit, lit_mom = ref.literal_two_steps(grad2d, count, t, th, True, noise, moments=moments)
    kind, offsets, out, mom = fused(t, grad2d, count, noise, th, True, mutant=mutant, moments=moments)
    good_kind, good_offsets, _, _ = fused(t, grad2d, count, noise, th, True)
    if mutant == "inclusive":
        assert np.array_equal(kind, good_kind) and not np.array_equal(offsets, good_offsets)
        assert not np.array_equal(np.diff(offsets), ref.ROWS_OUT[kind])  # a parent's rows no longer start where the one before ends
        return
    if mutant == "zero_original":
        # A clone and its original hold the same parameters, so as a multiset of rows the mutant looks like the rule: WHICH of the two
        # keeps the moments is a statement about positions.  The original is child 0, the row that stays where gsplat leaves it.
        new = ref.emit(kind, offsets, t["means"], t["scaling"], t["rotation"], t["opacity"], noise, th[4])
        k = kind[new["parent"]]
        want = moments[new["parent"]].copy()
        want[(k == ref.SPLIT) | ((k == ref.CLONE) & (new["child"] == 1))] = 0
        _, _, _, good_mom = fused(t, grad2d, count, noise, th, True, moments=moments)
        assert ((k == ref.CLONE) & (new["child"] == 0)).sum() > 10
        assert np.array_equal(good_mom, want) and not np.array_equal(mom, want)
        return
    assert not np.array_equal(kind, good_kind)
    assert ref.row_multiset(out) != ref.row_multiset(lit)


def test_split_children_against_the_float64_formula():
    """|float32 restatement - float64| <= 2^-21 (|mean_i| + 3 s |z|) on the same float32 inputs (densify_ref.split_bound)."""
    r = np.random.default_rng(11)
    n = 100_000
    means = ref.f32(r.normal(size=(n, 3)) * 3.0)
    scaling = ref.f32(math.log(0.05) + r.normal(size=(n, 3)))
    rotation = ref.f32(r.normal(size=(n, 4)))
    noise = ref.f32(r.normal(size=(n, 3)))
    m32 = ref.split_means(means, scaling, rotation, noise)
    m64 = ref.split_means(means, scaling, rotation, noise, dtype=np.float64)
    assert m32.dtype == np.float32 and m64.dtype == np.float64
    ratio = np.abs(m32.astype(np.float64) - m64) / ref.split_bound(means, scaling, noise)
    print(f"split children, float32 against float64: largest error / bound = {ratio.max():.3f}, median {np.median(ratio):.4f}")
    assert ratio.max() <= 1.0
    # the formula itself: an identity rotation moves the mean by exp(scaling) * noise, and a unit quaternion need not be normalised
    ident = np.tile(ref.f32([[3.0, 0.0, 0.0, 0.0]]), (n, 1))
    want = means.astype(np.float64) + np.exp(scaling.astype(np.float64)) * noise
    assert np.abs(ref.split_means(means, scaling, ident, noise, dtype=np.float64) - want).max() < 1e-12
    # a wrong sign in one entry of R is far outside the bound
    flipped = rotation.copy()
    flipped[:, 1] = -flipped[:, 1]
    off = np.abs(ref.split_means(means, scaling, flipped, noise).astype(np.float64) - m64) / ref.split_bound(means, scaling, noise)
    assert np.median(off) > 100.0


def test_accumulate_reference():
    r = np.random.default_rng(2)
    v = ref.f32(r.normal(size=(3, 50, 2)) * 1e-4)
    radii = r.integers(0, 3, size=(3, 50)).astype(np.int32)
    v[1, 7, 0] = np.nan
    radii[:, 7] = 1
    g, c = ref.accumulate(np.zeros(50), np.zeros(50), v, radii, 48.0 * 3, 32.0 * 3)
    assert np.array_equal(c, (radii > 0).sum(axis=0).astype(np.float32))
    assert np.isnan(g[7]) and np.isfinite(np.delete(g, 7)).all()
    want = (np.hypot(v[..., 0].astype(np.float64) * 144.0, v[..., 1].astype(np.float64) * 96.0) * (radii > 0)).sum(axis=0)
    assert np.allclose(np.delete(g, 7), np.delete(want, 7), rtol=1e-6)


# ---- the header on the host ------------------------------------------------------------------------------------------------------------
def test_densify_math_on_the_host(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (c++, g++, clang++) found")
    exe = str(tmp_path / "densify_host")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-o", exe,
                           os.path.join(ROOT, "tests", "densify_host.cpp")])
    t, grad2d, count, noise, th = scene(n=4001, seed=21)
    n = len(grad2d)
    r = np.random.default_rng(4)
    gx, gy = ref.f32(r.normal(size=n) * 1e-4), ref.f32(r.normal(size=n) * 1e-4)
    gx[:3], gy[:3] = [0.0, np.nan, 1e-30], [0.0, 1.0, 1e-30]
    t["opacity"][5] = np.nan
    t["scaling"][6, 1] = np.nan
    sx, sy = 48.0 * 2, 32.0 * 2
    for prune_big in (0, 1):
        with open(tmp_path / "in.bin", "wb") as f:
            f.write(struct.pack("<qi7f", n, prune_big, *th, sx, sy))
            for a in (grad2d, count, t["scaling"], t["opacity"], t["means"], t["rotation"], noise[:, 0], gx, gy):
                f.write(ref.f32(a).tobytes())
        subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
        raw = open(tmp_path / "out.bin", "rb").read()
        assert len(raw) == 4 * n * 8
        kind = np.frombuffer(raw, np.int32, n)
        norm = np.frombuffer(raw, np.float32, n, 4 * n)
        split = np.frombuffer(raw, np.float32, 3 * n, 8 * n).reshape(n, 3)
        exps = np.frombuffer(raw, np.float32, 3 * n, 20 * n).reshape(n, 3)
        want_kind, _ = ref.plan(grad2d, count, t["scaling"], t["opacity"], th, prune_big)
        assert np.array_equal(kind, want_kind) and set(kind) == {0, 1, 2, 3}
        want_norm, _ = ref.accumulate(np.zeros(n), np.zeros(n), np.stack([gx, gy], axis=1)[None], np.ones((1, n), np.int32), sx, sy)
        assert np.array_equal(norm.view(np.uint32)[~np.isnan(norm)], want_norm.view(np.uint32)[~np.isnan(want_norm)])
        assert np.array_equal(np.isnan(norm), np.isnan(want_norm)) and np.isnan(norm[1])
        # with this libm's exponentials the split is the restatement's, bit for bit; numpy's own exp agrees to an ulp
        want_split = ref.split_means(t["means"], t["scaling"], t["rotation"], noise[:, 0], exp_scaling=exps)
        fin = np.isfinite(want_split).all(axis=1)
        assert fin.sum() >= n - 1 and np.array_equal(split[fin].view(np.uint32), want_split[fin].view(np.uint32))
        with np.errstate(invalid="ignore"):
            once = np.exp(t["scaling"].astype(np.float64)).astype(np.float32)  # the restatement's own: rounded once
            ulp = np.abs(exps.astype(np.float64) - once.astype(np.float64)) / np.spacing(once).astype(np.float64)
        print(f"host expf against the once-rounded exponential: {np.mean(ulp[np.isfinite(ulp)] > 0):.4f} of the values differ")
        assert np.nanmax(ulp) <= 1.0


# ---- the C ABI: nothing here reaches a kernel --------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_the_library_exports_them():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gwbp.h")).read(), flags=re.S)
    for name in ("gwbp_densify_accumulate", "gwbp_densify_plan", "gwbp_densify_emit", "gwbp_densify_gather",
                 "gwbp_densify_plan_workspace_size"):
        assert re.search(rf"GWBP_API int {name}\s*\(", src), name
        assert name in _lib.ARGTYPES
    gsbp_amd.build()
    assert all(hasattr(_lib.lib(), n) for n in ("gwbp_densify_accumulate", "gwbp_densify_plan", "gwbp_densify_emit", "gwbp_densify_gather"))


def test_the_package_exports_the_feature():
    for name in ("densify", "DensifyState", "DensifyConfig", "train_scene", "reset_opacity", "init_splats_from_points"):
        assert callable(getattr(gsbp_amd, name)), name


def _fake():
    buf = (C.c_double * 64)()
    return buf, C.addressof(buf)


def test_capi_rejects_without_a_launch():
    lib = _lib.lib()
    buf, a = _fake()

    def message():
        return lib.gwbp_last_error_string().decode()

    def acc(n=4, c=1, v=a, radii=a, g=a, cnt=a + 64):
        return lib.gwbp_densify_accumulate(n, c, v, radii, 1.0, 1.0, g, cnt, None)
    assert acc(n=-1) == -1 and "Gaussians" in message()
    assert acc(n=1 << 31) == -1
    assert acc(c=0) == -1 and "n_cameras" in message()
    for null in ("v", "radii", "g", "cnt"):
        assert acc(**{null: None}) == -1 and "null" in message()
    assert acc(v=a + 4) == -1 and "8-B" in message()
    assert acc(g=a + 2) == -1 and acc(radii=a + 1) == -1
    assert acc(cnt=a) == -1 and "same array" in message()

    need = C.c_size_t(0)
    assert lib.gwbp_densify_plan_workspace_size(1000, C.byref(need)) == 0 and need.value == 8 * 4
    assert lib.gwbp_densify_plan_workspace_size(0, C.byref(need)) == 0 and need.value == 8
    assert lib.gwbp_densify_plan_workspace_size(65537, C.byref(need)) == 0 and need.value == 8 * 257
    assert lib.gwbp_densify_plan_workspace_size(-1, C.byref(need)) == -1 and lib.gwbp_densify_plan_workspace_size(4, None) == -1

    def plan(n=4, g=a, cnt=a, s=a, lds=3, o=a, kind=a, off=a, ws=a, ws_bytes=64):
        return lib.gwbp_densify_plan(n, g, cnt, s, lds, o, 1.0, 1.0, 1.0, 1.0, 1.0, 0, kind, off, ws, ws_bytes, None)
    assert plan(n=-2) == -1
    assert plan(lds=2) == -1 and "stride" in message()
    for null in ("g", "cnt", "s", "o", "kind", "off", "ws"):
        assert plan(**{null: None}) == -1 and "null" in message()
    assert plan(off=a + 4) == -1 and "8-B" in message()
    assert plan(ws=a + 4) == -1 and plan(s=a + 2) == -1
    assert plan(n=1000, ws_bytes=31) == -2 and "32" in message()

    def emit(n=4, n_out=4, kind=a, off=a, m=a, s=a + 64, q=a + 128, o=a + 192, z=a + 256, parent=a, child=a, om=a + 320, os_=a + 352,
             oq=a + 384, oo=a + 416):
        return lib.gwbp_densify_emit(n, n_out, kind, off, m, s, q, o, z, 1.0, parent, child, om, os_, oq, oo, None)
    assert emit(n=-1) == -1
    for n_out in (-1, 9):
        assert emit(n_out=n_out) == -1 and "disagrees with offsets" in message()
    for null in ("kind", "off", "m", "s", "q", "o", "z", "parent", "child", "om", "os_", "oq", "oo"):
        assert emit(**{null: None}) == -1 and "null" in message(), null
    assert emit(off=a + 4) == -1 and "8-B" in message()
    assert emit(m=a + 2) == -1 and emit(parent=a + 2) == -1 and emit(oo=a + 418) == -1
    assert emit(om=a) == -1 and "input" in message()

    def gather(n=4, n_out=4, w=3, t=a, ldt=3, parent=a + 64, child=a + 128, kind=a + 192, mode=0, out=a + 256, ldo=3):
        return lib.gwbp_densify_gather(n, n_out, w, t, ldt, parent, child, kind, mode, out, ldo, None)
    assert gather(n=-1) == -1
    assert gather(n_out=9) == -1 and "disagrees with offsets" in message()
    for w in (0, -1, 65537):
        assert gather(w=w) == -1 and "w must be" in message()
    assert gather(ldt=2) == -1 and gather(ldo=2) == -1 and "strides" in message()
    assert gather(mode=2) == -1 and "mode" in message()
    for null in ("t", "parent", "out"):
        assert gather(**{null: None}) == -1 and "null" in message()
    assert gather(mode=1, child=None) == -1 and gather(mode=1, kind=None) == -1
    assert gather(t=a + 2) == -1 and gather(out=a + 258) == -1 and gather(parent=a + 65) == -1 and "aligned" in message()
    assert gather(out=a) == -1 and "must not be the table" in message()
    # an empty new set is no error and launches nothing
    assert gather(n_out=0, t=None, parent=None, out=None) == 0 and emit(n=0, n_out=0, kind=None, off=None, m=None, s=None, q=None,
                                                                       o=None, z=None, parent=None, child=None, om=None, os_=None,
                                                                       oq=None, oo=None) == 0
    del buf


# ---- the Python layer without a device ---------------------------------------------------------------------------------------------
def test_means2d_grad_refuses_tables_the_blend_backward_cannot_read():
    z = torch.zeros(4, 3)
    args = (z, torch.zeros(4, 4), z, torch.zeros(4))
    cams = (torch.eye(4)[None], torch.eye(3)[None], 64, 64)
    for table in (torch.zeros(4, 48), torch.zeros(4, 3, dtype=torch.float16), torch.zeros(4, 3, dtype=torch.bfloat16)):
        with pytest.raises(NotImplementedError, match="means2d_grad"):
            gsbp_amd.rasterization(*args, table, *cams, means2d_grad=True)
    with pytest.raises(NotImplementedError, match="means2d_grad"):
        gsbp_amd.rasterization(*args, torch.zeros(4, 32), *cams, means2d_grad=True, render_mode="RGB+D")  # 33 with the depth column
    with torch.no_grad():  # the keyword asks for nothing without grad mode: the call goes on to its own refusal of CPU tensors
        with pytest.raises(gsbp_amd.GwbpError, match="HIP tensors"):
            gsbp_amd.rasterization(*args, torch.zeros(4, 48), *cams, means2d_grad=True)
    with pytest.raises(NotImplementedError):
        gsbp_amd.rasterization(*args, z, *cams, absgrad=True)


def test_config_validation_and_thresholds():
    cfg = gsbp_amd.DensifyConfig()
    assert (cfg.prune_opa, cfg.grow_grad2d, cfg.grow_scale3d, cfg.prune_scale3d) == (0.005, 2e-4, 0.01, 0.1)
    assert (cfg.refine_start_iter, cfg.refine_stop_iter, cfg.refine_every, cfg.reset_every) == (500, 15000, 100, 3000)
    assert (cfg.pause_refine_after_reset, cfg.scene_scale, cfg.max_gaussians) == (0, 1.0, None)
    t = gsbp_amd.DensifyConfig(scene_scale=2.0).thresholds()
    want = (2e-4, math.log(0.02), math.log(0.2), math.log(0.005 / 0.995), math.log(1.6))
    assert all(a == float(np.float32(b)) for a, b in zip(t, want))
    for bad in (dict(prune_opa=0.0), dict(prune_opa=0.5), dict(grow_grad2d=-1.0), dict(grow_grad2d=float("nan")), dict(grow_scale3d=0.0),
                dict(prune_scale3d=-1.0), dict(scene_scale=float("inf")), dict(refine_every=0), dict(reset_every=0),
                dict(refine_start_iter=-1), dict(pause_refine_after_reset=-1), dict(max_gaussians=0)):
        with pytest.raises(gsbp_amd.GwbpError):
            gsbp_amd.DensifyConfig(**bad)
    cfg = gsbp_amd.DensifyConfig(refine_start_iter=10, refine_every=10, reset_every=40, pause_refine_after_reset=15, refine_stop_iter=100)
    assert [s for s in range(120) if cfg.refines_at(s)] == [20, 30, 60, 70]
    assert [s for s in range(130) if cfg.resets_at(s)] == [40, 80]


def test_cpu_tensors_raise():
    sc = gsbp_amd.synthetic.make_scene(gsbp_amd.synthetic.CONFIGS["T0"])
    sc["features_dc"] = torch.zeros(512, 1, 3)
    cfg = gsbp_amd.DensifyConfig()
    with pytest.raises(gsbp_amd.GwbpError, match="no CPU path"):
        gsbp_amd.DensifyState(512, "cpu")
    with pytest.raises(gsbp_amd.GwbpError, match="no CPU path"):
        gsbp_amd.densify(sc, None, cfg, 600)
    with pytest.raises(gsbp_amd.GwbpError, match="no CPU path"):
        gsbp_amd.train_scene(sc, torch.eye(4)[None], torch.eye(3), 96, 64, lambda v: None, 10, cfg)
    with pytest.raises(gsbp_amd.GwbpError, match="no CPU path"):
        gsbp_amd.init_splats_from_points(torch.zeros(8, 3), torch.zeros(8, 3))
    with pytest.raises(gsbp_amd.GwbpError, match="params"):
        gsbp_amd.train_scene(sc, torch.eye(4)[None], torch.eye(3), 96, 64, lambda v: None, 10, cfg, params=("colours",))
