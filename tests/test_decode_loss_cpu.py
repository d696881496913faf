"""No-GPU checks of the decode-loss feature: the numpy reference (tests/decode_ref.py) against torch.autograd on the literal
expression in float64, the properties its GPU tests lean on (the l1 margin, the share of sensitive Gaussians, the fit loop's
float32-vs-float64 margin), the C ABI's argument checks, and the checkpoint keys."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import gsbp_amd
from gsbp_amd import _lib
from gsbp_amd import scene_io as sio
from gsbp_amd import synthetic as syn

import decode_ref as ref
import fidelity_ref as fid
from test_scene_io import _write_colmap


def _autograd(R, C_, M, loss, scale, weights, keep):
    """loss and gradients of the literal expression on the rows `keep` (torch cannot skip a non-finite row by itself)."""
    r = torch.tensor(R, dtype=torch.float64, requires_grad=True)
    c = torch.tensor(C_, dtype=torch.float64, requires_grad=True)
    m = torch.tensor(np.asarray(M, np.float64)[keep])
    e = (r @ c)[torch.from_numpy(keep)] - m
    t = e.abs() if loss == "l1" else e * e
    if weights is not None:
        t = t * torch.tensor(np.asarray(weights, np.float64)[keep])[:, None]
    total = scale * t.sum()
    total.backward()
    return float(total.detach()), r.grad.numpy(), c.grad.numpy()


@pytest.mark.parametrize("loss", ["l1", "l2"])
def test_reference_equals_autograd_of_the_literal_expression(loss):
    P, d, D = 37, 16, 48
    R, C_, M = ref.kernel_inputs(P, d, D, seed=2, loss=loss)
    weights = np.random.default_rng(4).uniform(0.0, 2.0, P)
    weights[5] = 0.0
    for w in (None, weights):
        for bad_row in (None, 11):
            m = M.copy()
            if bad_row is not None:
                m[bad_row, 3] = np.inf
                m[bad_row + 1, D - 1] = np.nan
            keep = np.isfinite(m).all(axis=1)
            got = ref.reference(R, C_, m, loss, 0.125, w)
            want = _autograd(R, C_, m, loss, 0.125, w, keep)
            assert got["n_bad"] == (0 if bad_row is None else 2)
            assert got["loss"] == pytest.approx(want[0], rel=1e-12)
            np.testing.assert_allclose(got["GR"], want[1], rtol=1e-11, atol=1e-13)
            np.testing.assert_allclose(got["GC"], want[2], rtol=1e-11, atol=1e-13)
            assert not got["GR"][~keep].any()
    # mean reduction: F.l1_loss / F.mse_loss themselves
    f = torch.nn.functional.l1_loss if loss == "l1" else torch.nn.functional.mse_loss
    r, c = torch.tensor(R, dtype=torch.float64), torch.tensor(C_, dtype=torch.float64)
    assert ref.reference(R, C_, M, loss, 1.0 / (P * D))["loss"] == pytest.approx(float(f(r @ c, torch.tensor(M, dtype=torch.float64))),
                                                                                 rel=1e-12)


def test_l1_map_keeps_every_error_away_from_zero():
    """No |e| within 0.05 mean |y| of zero in float64 -- and the fp32 bound on y, (d + 2) 2^-24 |R| |C|, is far below that margin,
    so no sign can flip on the GPU."""
    for P, d, D in ((70 * 45, 128, 80), (64, 16, 1040)):
        R, C_, M = ref.kernel_inputs(P, d, D, seed=0, loss="l1")
        out = ref.reference(R, C_, M, "l1")
        margin = 0.05 * np.abs(out["y"]).mean()
        assert np.abs(out["e"]).min() >= 0.99 * margin  # (0.99: M was rounded to float32)
        assert ((d + 2) * ref.U * out["y_abs"]).max() < 0.01 * margin
    latents, conv, M, margin = ref.view_case()
    out = ref.reference(fid.render64(fid.pairs(0), latents), conv, M.reshape(ref.H * ref.W, -1), "l1")
    assert np.abs(out["e"]).min() >= 0.99 * margin


def test_sensitive_gaussians_of_the_reference_scene_stay_under_one_percent(orc):
    latents, conv, M, _ = ref.view_case()
    for loss in ("l1", "l2"):
        sens, live = ref.sensitive_gaussians(0, latents, conv, M, loss)
        print(f"{loss}: {int((sens & live).sum())} sensitive of {int(live.sum())} Gaussians with a gradient")
        assert live.sum() > 0.3 * ref.N and (sens & live).sum() <= 0.01 * live.sum()


def test_literal_fit_loop_converges_and_its_float32_history_stays_within_the_margin(orc):
    h32, h64 = ref.literal_fit(torch.float32), ref.literal_fit(torch.float64)
    rel = max(abs(a - b) / b for a, b in zip(h32, h64))
    print(f"literal fit: loss {h64[0]:.6e} -> {h64[-1]:.6e}; largest per-step relative float32 / float64 difference {rel:.3e}")
    assert len(h64) == ref.FIT_STEPS and h64[-1] < h64[0]
    assert rel <= 2 * ref.FIT_F32_VS_F64  # the recorded figure (this host's float32 matmul may round differently: a factor 2)
    assert ref.fit_margin() == pytest.approx(10 * rel)


def _fake():
    buf = (C.c_char * 512)()
    return buf, C.c_void_p((C.addressof(buf) + 255) & ~255)


def _call(lib, fake, **over):
    a = dict(height=4, width=4, d=16, D=16, R=fake, ldr=16, C=fake, ldc=16, map=fake, mt=_lib.MAP_F32, ms_y=64, ms_x=16, pw=None,
             kind=0, scale=1.0, GR=fake, ldg=16, GC=fake, ldgc=16, table=fake, ws=fake, bytes=1 << 30, stream=None)
    a.update(over)
    return lib.gwbp_decode_loss(*a.values())


def test_abi_argument_checks_need_no_device():
    gsbp_amd.build()
    lib = _lib.lib()
    keep, fake = _fake()
    n = C.c_size_t(0)
    assert lib.gwbp_decode_loss_workspace_size(128, 512, C.byref(n)) == 0
    assert n.value == 512 * (128 * 512 * 4 + 16)  # the slices' partials: d and D alone
    for d in (0, 8, 24, 144):
        assert _call(lib, fake, d=d) == -3 and b"d must be" in lib.gwbp_last_error_string()
        assert lib.gwbp_decode_loss_workspace_size(d, 64, C.byref(n)) == -3
    for D in (0, 8, 40, 2064):
        assert _call(lib, fake, D=D) == -3 and b"D must be" in lib.gwbp_last_error_string()
    assert _call(lib, fake, height=8192, width=8192) == -3 and b"pixels" in lib.gwbp_last_error_string()
    for name in ("R", "C", "map", "GR", "GC", "table", "ws"):
        assert _call(lib, fake, **{name: None}) == -1 and b"null" in lib.gwbp_last_error_string(), name
    assert _call(lib, fake, mt=7) == -1 and b"map type" in lib.gwbp_last_error_string()
    assert _call(lib, fake, kind=2) == -1 and b"loss kind" in lib.gwbp_last_error_string()
    assert _call(lib, fake, ldr=8) == -1 and b"row strides" in lib.gwbp_last_error_string()
    assert _call(lib, fake, ms_x=-1) == -1 and b"negative map strides" in lib.gwbp_last_error_string()
    assert _call(lib, fake, R=C.c_void_p(fake.value + 2)) == -1 and b"aligned" in lib.gwbp_last_error_string()
    assert _call(lib, fake, table=C.c_void_p(fake.value + 4)) == -1 and b"8-B" in lib.gwbp_last_error_string()
    assert _call(lib, fake, bytes=1024) == -2 and b"workspace has" in lib.gwbp_last_error_string()
    pw = _lib.PixelWeights()
    pw.data, pw.dtype = fake.value, 9
    assert _call(lib, fake, pw=C.byref(pw), d=8) == -1 and b"pixel weight type" in lib.gwbp_last_error_string()  # before the shape
    assert lib.gwbp_decode_loss_workspace_size(16, 16, None) == -1
    del keep


def test_python_entry_points_refuse_cpu_tensors():
    r, c, m = torch.zeros(4, 4, 16), torch.zeros(16, 16), torch.zeros(4, 4, 16)
    with pytest.raises(gsbp_amd.GwbpError):
        gsbp_amd.decoded_loss(r, c, m)
    with pytest.raises(gsbp_amd.GwbpError):
        gsbp_amd.fit_decoded_field(torch.zeros(4, 3), None, None, None, None, None, 4, 4, None, 16)
    assert torch.equal(gsbp_amd.decode_field(torch.ones(3, 16), torch.ones(16, 32)), torch.full((3, 32), 16.0))


def test_load_checkpoint_keeps_features_and_conv(tmp_path):
    cfg = syn.CONFIGS["T0"]
    K = syn.intrinsics(cfg).numpy().astype(np.float64)
    data_dir = str(tmp_path / "scene")
    _write_colmap(os.path.join(data_dir, "sparse", "0"), K, syn.make_cameras(cfg, n_views=2).numpy(), ["a.png", "b.png"],
                  cfg.width, cfg.height)
    sc = syn.make_scene(cfg)
    n = cfg.n_gaussians
    p = {"means": sc["means"], "sh0": torch.zeros(n, 1, 3), "shN": torch.zeros(n, 15, 3), "scales": sc["scaling"],
         "quats": sc["rotation"], "opacities": sc["opacity"]}
    path = str(tmp_path / "ckpt.pt")
    torch.save({"splats": p}, path)
    plain = sio.load_checkpoint(path, data_dir, format="gsplat")
    assert "features" not in plain and "conv" not in plain
    feats, conv = torch.randn(n, 128, requires_grad=True), torch.rand(128, 512)
    torch.save({"splats": dict(p, features=feats, conv=conv)}, path)
    got = sio.load_checkpoint(path, data_dir, format="gsplat")
    assert set(got) == set(plain) | {"features", "conv"}
    assert torch.equal(got["features"], feats.detach()) and not got["features"].requires_grad and torch.equal(got["conv"], conv)
    assert all(torch.equal(got[k], plain[k]) for k in ("means", "scaling", "rotation", "opacity"))
