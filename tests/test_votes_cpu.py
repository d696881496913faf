"""No-GPU checks of the per-view votes (gwbp_vote_labels, gwbp_vote_projected, Engine.vote_labels / vote_projected,
create_vote_field, mask3d_from_votes, run_backproject.py --votes): the C ABI and its argument validation, the numpy restatement of
both votes against literal loops on the CPU oracle, the rounding rule, and a cross-compile of the kernels."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from votes_ref import (binary_votes, binary_votes_loop, oracle_view, projection_votes, projection_votes_loop)

import gsbp_amd
from gsbp_amd import _lib, mask3d_from_votes
from gsbp_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOTES = ("gwbp_vote_labels", "gwbp_vote_projected")


def test_votes_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "gwbp.h")).read()
    for name in VOTES:
        assert f"GWBP_API int {name}(" in hdr
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in VOTES:
        assert name in exported and name in _lib.EXPORTS
    assert "gwbp_*" in open(os.path.join(ROOT, "3dgs-gradient-backprojection_amd", "csrc", "gwbp.map")).read()


def _vote_labels(label_type=_lib.LABEL_I32, K=4, ldc=4, Cp=True, ymap=False, xmap=False, seen=True, seen_off=0):
    """gwbp_vote_labels with NULL caps, workspace and view: only the vote arguments can be looked at before the caps."""
    buf = (C.c_char * 64)()
    fake = C.c_void_p(C.addressof(buf))
    s = C.c_void_p(C.addressof(buf) + seen_off) if seen else None
    return _lib.lib().gwbp_vote_labels(None, None, 0, None, fake, label_type, 1, 1, fake if ymap else None, fake if xmap else None,
                                       K, s, fake if Cp else None, ldc, None, None)


def _vote_projected(label_type=_lib.LABEL_I32, K=4, ldc=4, Cp=True, ymap=False, xmap=False, pw=None, ls=1):
    buf = (C.c_char * 64)()
    fake = C.c_void_p(C.addressof(buf))
    return _lib.lib().gwbp_vote_projected(None, None, 0, None, fake, label_type, ls, 1, fake if ymap else None,
                                          fake if xmap else None, C.byref(pw) if pw is not None else None, K,
                                          fake if Cp else None, ldc, None, None)


@pytest.mark.parametrize("kw, msg", [
    (dict(label_type=3), b"unknown label type"),
    (dict(K=0, ldc=0), b"num_classes must be positive"),
    (dict(K=8, ldc=7), b"ldc"),
    (dict(Cp=False), b"null C"),
    (dict(ymap=True), b"both index maps or neither"),
    (dict(seen=False), b"seen must be"),
    (dict(seen_off=2), b"seen must be"),
])
def test_vote_labels_arguments_are_einval_before_any_device_call(kw, msg):
    assert _vote_labels(**kw) == -1  # GWBP_EINVAL
    assert msg in _lib.lib().gwbp_last_error_string()


def test_vote_projected_arguments_are_einval_before_any_device_call():
    assert _vote_projected(label_type=7) == -1 and b"unknown label type" in _lib.lib().gwbp_last_error_string()
    assert _vote_projected(xmap=True) == -1 and b"both index maps" in _lib.lib().gwbp_last_error_string()
    assert _vote_projected(ls=-1) == -1 and b"bad label map" in _lib.lib().gwbp_last_error_string()
    bad = _lib.PixelWeights(None, 0, 0, _lib.PIXW_F32, 0)
    assert _vote_projected(pw=bad) == -1 and b"null pixel weight map" in _lib.lib().gwbp_last_error_string()


def test_valid_vote_arguments_reach_the_caps_check():
    assert _vote_labels(ymap=True, xmap=True) == -1 and b"null caps" in _lib.lib().gwbp_last_error_string()
    assert _vote_projected() == -1 and b"null caps" in _lib.lib().gwbp_last_error_string()


def test_vote_words():
    assert [gsbp_amd.Engine.vote_words(k) for k in (1, 2, 30, 31, 32, 63, 64, 1000)] == [1, 1, 1, 1, 2, 2, 3, 32]


@pytest.fixture(scope="module")
def t0_views(orc):
    cfg = syn.CONFIGS["T0"]
    means, quats, scales, opac = (t.numpy() for t in syn.activate(syn.make_scene(cfg)))
    K, vms = syn.intrinsics(cfg).numpy(), syn.make_cameras(cfg).numpy()
    return cfg, [oracle_view(orc, means, quats, scales, opac, vms[v], K, cfg.width, cfg.height) for v in range(cfg.n_views)]


@pytest.mark.parametrize("K, per_pixel", [(2, False), (5, False), (40, True)])
def test_numpy_votes_equal_literal_loops(t0_views, K, per_pixel):
    cfg, views = t0_views
    N = cfg.n_gaussians
    for v, (proj, gid, pix, w) in enumerate(views):
        L = (syn.make_label_map(cfg, v, K + 2, per_pixel=per_pixel) - 1).numpy()  # ids -1 and K are ignored
        assert gid.size > 0
        Cb, nb = binary_votes(gid, pix, w, L, K, N)
        Cl, nl = binary_votes_loop(gid, pix, w, L, K, N)
        assert np.array_equal(Cb, Cl) and np.array_equal(nb, nl) and nb.sum() > 0
        assert (Cb.sum(1) <= K * nb).all() and (Cb.max(1) <= nb).all()
        Cp, np_ = projection_votes(proj["means2d"], proj["radii"], L, K)
        Cq, nq = projection_votes_loop(proj["means2d"], proj["radii"], L, K)
        assert np.array_equal(Cp, Cq) and np.array_equal(np_, nq) and np_.sum() > 0
        assert (Cp.sum(1) <= np_).all()  # one vote per view, for at most one label


def test_pixel_weights_of_zero_remove_pairs(t0_views):
    cfg, views = t0_views
    proj, gid, pix, w = views[0]
    L = syn.make_label_map(cfg, 0, 3).numpy()
    c = (syn.make_pixel_weights(cfg, 0, kind="mask").numpy() != 0).astype(np.float32)
    Cw, nw = binary_votes(gid, pix, w, L, 3, cfg.n_gaussians, weights=c)
    keep = c.reshape(-1)[pix] > 0
    Cr, nr = binary_votes_loop(gid[keep], pix[keep], w[keep], L, 3, cfg.n_gaussians)
    assert np.array_equal(Cw, Cr) and np.array_equal(nw, nr)


def test_rounding_is_half_to_even_like_np_round():
    """The projection vote rounds with rintf, i.e. half to even -- the rule of np.round (get_mask3d), of Python's round() and of
    torch.round, and not the half-away-from-zero of C's roundf."""
    x = np.array([-1.5, -0.5, 0.5, 1.5, 2.5, 3.5, 10.5, 11.5, 2.4999998, 2.5000002, -0.49999997], np.float32)
    want = np.array([-2, -0, 0, 2, 2, 4, 10, 12, 2, 3, -0], np.float32)
    assert np.array_equal(np.round(x), want) and np.array_equal(np.rint(x), want)
    assert [round(float(t)) for t in x] == want.astype(int).tolist()
    assert torch.equal(torch.round(torch.from_numpy(x)), torch.from_numpy(want))
    # -0.5 rounds to -0.0, which is inside [0, W): a centre half a pixel left of the image still votes for column 0
    assert np.round(np.float32(-0.5)) >= 0


def test_mask3d_from_votes():
    C = torch.tensor([[0., 3.], [2., 1.], [1., 1.], [0., 0.], [4., 5.]])
    m, mi = mask3d_from_votes(C)
    assert m.tolist() == [True, False, False, False, True] and mi.tolist() == [False, True, False, False, False]
    m2, mi2 = mask3d_from_votes(C, positive=0, negative=1)
    assert torch.equal(m2, mi) and torch.equal(mi2, m)
    C3 = torch.tensor([[1., 0., 2.], [0., 5., 1.]])
    assert mask3d_from_votes(C3, positive=2, negative=1)[0].tolist() == [True, False]
    for kw in (dict(positive=2), dict(negative=-1), dict(positive=0), dict(positive=True), dict(positive=1.0)):
        with pytest.raises(ValueError):
            mask3d_from_votes(C, **kw)
    with pytest.raises(ValueError):
        mask3d_from_votes(C[:, 0])


def test_create_vote_field_rejects_bad_arguments_before_the_device():
    cfg = syn.CONFIGS["T0"]
    means, quats, scales, opac = syn.activate(syn.make_scene(cfg))
    K, vms = syn.intrinsics(cfg), syn.make_cameras(cfg)
    args = (means, quats, scales, opac, vms, K, cfg.width, cfg.height, lambda v: None)
    with pytest.raises(ValueError, match="method"):
        gsbp_amd.create_vote_field(*args, 2, method="soft")
    with pytest.raises(ValueError, match="upsample"):
        gsbp_amd.create_vote_field(*args, 2, upsample="bilinear")
    with pytest.raises(ValueError, match="num_classes"):
        gsbp_amd.create_vote_field(*args, 0)


def _cli():
    sys.path.insert(0, ROOT)
    import run_backproject
    return run_backproject


def test_cli_votes_flag_parses_and_needs_label_maps():
    rb = _cli()
    p = rb.build_parser()
    a = p.parse_args(["--synthetic", "C1", "--num-classes", "2", "--votes", "binary"])
    assert a.votes == "binary" and a.num_classes == 2
    assert p.parse_args([]).votes is None
    with pytest.raises(SystemExit):
        p.parse_args(["--votes", "soft"])
    with pytest.raises(SystemExit):  # --votes without label maps: refused before anything touches the device
        rb.main(["--synthetic", "C1", "--votes", "projection"])


def test_votes_kernels_cross_compile_for_gfx950(tmp_path):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not installed")
    src = os.path.join(ROOT, "3dgs-gradient-backprojection_amd", "csrc", "votes.hip")
    asm = tmp_path / "votes.s"
    subprocess.run([hipcc, "-std=c++17", "-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-munsafe-fp-atomics",
                    "--cuda-device-only", "-S", "-o", str(asm), src], check=True, capture_output=True)
    text = asm.read_text()
    for k in ("k_vote_labels", "k_vote_commit", "k_vote_projected"):
        assert re.search(rf"\.name:\s+\S*{k}", text), k
    assert "global_atomic_or" in text and "v_rndne_f32" in text
