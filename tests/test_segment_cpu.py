"""No-GPU checks of prompt segmentation: the float64 reference's own conditions on the committed cases, the host logic of
gsbp_amd.segment, the C-ABI validation of gwbp_prompt_scores / gwbp_probe_pixels and the shape of the two kernels' assembly."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import gsbp_amd
from gsbp_amd import _lib, segment as seg

import ref_np
import segment_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the cases decide almost every row -------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("case", ref.CASES, ids=[f"N{c[0]}-D{c[1]}-P{c[2]}-pos{c[3]}" for c in ref.CASES])
def test_reference_decides_all_but_one_percent_of_the_rows(case, normalize):
    n, d, p, n_pos = case
    x, t = ref.make_case(*case)
    s, b = ref.scores(x, t, normalize), ref.bound(x, t, normalize)
    und = 1.0 - ref.decided(s, b, n_pos).mean()
    pos = ref.mask_of(s, n_pos).mean()
    print(f"{case} normalize={normalize}: undecided {100 * und:.3f} %, positive {100 * pos:.1f} %")
    assert und <= 0.01
    assert 0.05 <= pos <= 0.95
    # with a threshold between the two modes of prompt 0's scores, and in the no-negatives form
    thr = ref.threshold_of(s)
    assert 1.0 - ref.decided(s, b, n_pos, thr).mean() <= 0.01
    assert 1.0 - ref.decided(s[:, :n_pos], b[:, :n_pos], n_pos, thr).mean() <= 0.01
    assert 0.05 <= ref.mask_of(s[:, :n_pos], n_pos, thr).mean() <= 0.95


# ---- 2. the 2-D mask of a small scene ------------------------------------------------------------------------------------------
def pixel_margins(scene, prompts, n_pos):
    """(margin [H W], slack [H W], covered [H W], mask [H W]) of the P-channel render of the unnormalised scores in float64: a pixel
    is decided when margin > slack = sum_g w 2 max_j B[g, j] + (n + 2) u max_j sum_g w |s[g, j]|, n = its contributing Gaussians."""
    W, H = scene["width"], scene["height"]
    proj = ref_np.project(scene["means"], scene["quats"], scene["scales"], scene["viewmat"], scene["K"], W, H)
    Wm, _ = ref_np.weights(proj, scene["opac"].astype(np.float64), W, H)
    s, b = ref.scores(scene["feats"], prompts, False), ref.bound(scene["feats"], prompts, False)
    r = Wm @ s
    margin = np.abs(r[:, :n_pos].max(axis=1) - r[:, n_pos:].max(axis=1))
    n = (Wm > 0).sum(axis=1)
    slack = Wm @ (2.0 * b.max(axis=1)) + (n + 2) * ref.U * (Wm @ np.abs(s)).max(axis=1)
    return margin, slack, n > 0, ref.mask_of(r, n_pos)


def test_reference_decides_all_but_one_percent_of_the_pixels():
    scene = ref.two_blob_scene(n_per=60)
    rng = np.random.default_rng(5)
    prompts = (scene["feats"][[0, 60]] + 0.02 * rng.standard_normal((2, scene["feats"].shape[1]))).astype(np.float32)
    margin, slack, covered, mask = pixel_margins(scene, prompts, 1)
    und = ((margin <= slack) & covered).sum() / covered.sum()
    pos = mask[covered].mean()
    print(f"covered {covered.sum()} pixels, undecided {100 * und:.3f} %, positive {100 * pos:.1f} %")
    assert covered.sum() > 500 and und <= 0.01 and 0.05 <= pos <= 0.95


# ---- 3. host logic ---------------------------------------------------------------------------------------------------------------
def test_click_session_bookkeeping():
    f = torch.randn(10, 6)
    s = seg.ClickSession(f, negatives=torch.randn(2, 6))
    assert s.mask() is None and s.prompts()[1] == 0 and s.prompts()[0].shape == (2, 6)
    a, b = torch.randn(6), torch.randn(6)
    assert s.add_positive(a, position=(1.0, 2.0, 3.0)) == 0 and s.add_positive(b) == 1
    assert s.add_negative(torch.randn(1, 6), position="n") == 2
    t, n_pos = s.prompts()
    assert t.shape == (5, 6) and n_pos == 2 and torch.equal(t[0], a) and torch.equal(t[1], b)
    assert s.positive_positions == [(1.0, 2.0, 3.0), None] and s.negative_positions == [None, None, "n"]
    s.remove_positive(0)
    s.remove_negative(0)
    t, n_pos = s.prompts()
    assert t.shape == (3, 6) and n_pos == 1 and torch.equal(t[0], b) and s.positive_positions == [None]
    a += 1.0  # the session keeps its own copy
    with pytest.raises(gsbp_amd.GwbpError):
        s.add_positive(torch.randn(5))
    with pytest.raises(gsbp_amd.GwbpError):  # no CPU path: a mask needs the device
        s.mask()
    s.remove_positive(0)
    assert s.mask() is None
    full = seg.ClickSession(f)
    for _ in range(seg.MAX_P):
        full.add_negative(torch.randn(6))
    with pytest.raises(gsbp_amd.GwbpError):
        full.add_positive(torch.randn(6))


def test_apply_mask3d_cuts_every_per_gaussian_tensor():
    n = 7
    splats = dict(means=torch.randn(n, 3), scaling=torch.randn(n, 3), rotation=torch.randn(n, 4), opacity=torch.randn(n),
                  features_dc=torch.randn(n, 1, 3), features_rest=torch.randn(n, 15, 3), camera_matrix=torch.eye(3), other="x")
    mask = torch.tensor([True, False, True, True, False, False, False])
    ext, dele = seg.apply_mask3d(splats, mask)
    for k in ("means", "scaling", "rotation", "opacity", "features_dc", "features_rest"):
        assert ext[k].shape[0] == 3 and dele[k].shape[0] == 4 and ext[k].shape[1:] == splats[k].shape[1:]
        assert torch.equal(ext[k], splats[k][mask]) and torch.equal(dele[k], splats[k][~mask])
    assert ext["camera_matrix"] is splats["camera_matrix"] and dele["other"] == "x" and splats["means"].shape[0] == n
    with pytest.raises(gsbp_amd.GwbpError):
        seg.apply_mask3d(splats, mask[:-1])
    with pytest.raises(gsbp_amd.GwbpError):
        seg.apply_mask3d(splats, mask.to(torch.uint8))
    ck = seg.checkpoint_layout(ext)
    assert sorted(ck["splats"]) == ["means", "opacities", "quats", "scales", "sh0", "shN"] and ck["splats"]["shN"].shape == (3, 15, 3)


def test_file_formats_round_trip(tmp_path):
    t = torch.randn(4, 8)
    seg.save_prompts(str(tmp_path / "p.pt"), t, 3)
    back, n_pos = seg.load_prompts(str(tmp_path / "p.pt"))
    assert torch.equal(back, t) and n_pos == 3
    torch.save({"prompts": t}, tmp_path / "bad.pt")
    with pytest.raises(gsbp_amd.GwbpError):
        seg.load_prompts(str(tmp_path / "bad.pt"))
    torch.save({"prompts": t, "n_pos": 5}, tmp_path / "bad2.pt")
    with pytest.raises(gsbp_amd.GwbpError):
        seg.load_prompts(str(tmp_path / "bad2.pt"))
    mask = torch.rand(100) > 0.5
    torch.save(mask, tmp_path / "mask3d.pt")
    assert torch.equal(torch.load(tmp_path / "mask3d.pt"), mask) and torch.load(tmp_path / "mask3d.pt").dtype == torch.bool


def test_encoder_multiplies_and_renormalises():
    p, e = torch.randn(3, 32), torch.randn(32, 8)
    out = seg.encode_prompts(p, e)
    want = p.double() @ e.double()
    want = want / want.norm(dim=1, keepdim=True)
    assert out.shape == (3, 8) and torch.allclose(out.double(), want, atol=1e-5)
    assert torch.allclose(out.norm(dim=1), torch.ones(3), atol=1e-6)
    with pytest.raises(gsbp_amd.GwbpError):
        seg.encode_prompts(p, torch.randn(16, 8))


def test_overlay_is_the_reference_formula():
    frame = torch.randint(0, 256, (5, 7, 3), dtype=torch.uint8)
    mask = torch.rand(5, 7) > 0.5
    m = mask[..., None].numpy()
    want = frame.numpy() * (0.75 + 0.25 * m * np.array([255, 0, 0]) + (1 - m) * 0.25)
    want = np.clip(want, 0, 255).astype(np.uint8)
    assert np.array_equal(seg.overlay(frame, mask).numpy(), want)


def test_mask_from_scores_follows_torch_max():
    s = torch.tensor([[1.0, 0.5, 0.2], [0.1, 0.5, 0.2], [float("nan"), 0.0, 0.0], [1.0, float("nan"), 0.0]])
    assert seg.mask_from_scores(s, 1).tolist() == [True, False, False, False]
    assert seg.mask_from_scores(s, 1, threshold=2.0).tolist() == [False] * 4
    assert seg.mask_from_scores(s[:, :1], 1, threshold=0.5).tolist() == [True, False, False, True]
    with pytest.raises(gsbp_amd.GwbpError):
        seg.mask_from_scores(s, 3)


def test_python_layer_refuses_cpu_tensors_and_bad_sizes():
    f = torch.randn(8, 4)
    with pytest.raises(gsbp_amd.GwbpError):
        gsbp_amd.prompt_scores(f, torch.randn(2, 4))
    with pytest.raises(gsbp_amd.GwbpError):
        gsbp_amd.probe_pixels(f[:, :3], f, f[:, :3], f[:, 0], f, torch.eye(4), torch.eye(3), 8, 8, [[1, 1]])


# ---- 4. C ABI validation, before any HIP call ---------------------------------------------------------------------------------
def test_prompt_scores_validates_before_any_device_call():
    L = _lib.lib()
    buf = (C.c_char * 512)()
    fake = C.c_void_p((C.addressof(buf) + 255) & ~255)
    odd = C.c_void_p(fake.value + 2)
    thr = C.byref(C.c_float(0.5))

    def call(N=8, D=4, P=3, n_pos=1, X=fake, ldx=4, T=fake, norm=1, th=None, mask=fake, scores=fake):
        return L.gwbp_prompt_scores(N, D, P, n_pos, X, ldx, T, norm, th, mask, scores, None)

    for kw, msg in ((dict(N=-1), b"N must not be negative"), (dict(P=0), b"P must be in [1, 32]"), (dict(P=33), b"P must be in [1, 32]"),
                    (dict(n_pos=0), b"n_pos must be in [1, P = 3]"), (dict(n_pos=4), b"n_pos must be in [1, P = 3]"),
                    (dict(D=0), b"D must be in [1, 2048]"), (dict(D=2049, ldx=4096), b"D must be in [1, 2048]"),
                    (dict(ldx=3), b"row stride 3 below D = 4"), (dict(X=None), b"null X"), (dict(X=odd), b"X must be 4-B aligned"),
                    (dict(T=None), b"prompts must be a non-null"), (dict(T=odd), b"prompts must be a non-null"),
                    (dict(mask=None, scores=None), b"both null"), (dict(scores=odd), b"scores must be 4-B aligned"),
                    (dict(n_pos=3), b"needs a threshold"), (dict(P=1, n_pos=1), b"needs a threshold")):
        assert call(**kw) == -1, kw
        assert msg in L.gwbp_last_error_string(), (kw, L.gwbp_last_error_string())
    # N == 0 is valid and launches nothing; so is the no-negatives form that only asks for scores
    assert call(N=0) == 0 and call(N=0, n_pos=3, th=thr) == 0 and call(N=0, n_pos=3, mask=None) == 0


def test_probe_pixels_validates_its_own_arguments_before_the_workspace():
    L = _lib.lib()
    buf = (C.c_char * 512)()
    fake = C.c_void_p((C.addressof(buf) + 255) & ~255)
    odd = C.c_void_p(fake.value + 2)

    def call(M=4, xy=fake, X=fake, ldx=4, D=4, out=fake, depth=fake, alpha=fake):  # NULL caps: the next thing looked at
        return L.gwbp_probe_pixels(None, None, 0, None, M, xy, X, ldx, D, out, depth, alpha, None)

    for kw, msg in ((dict(M=0), b"M must be in [1, 4096]"), (dict(M=4097), b"M must be in [1, 4096]"),
                    (dict(D=0), b"D must be in [1, 2048]"), (dict(ldx=3), b"row stride 3 below D = 4"), (dict(X=None), b"null X"),
                    (dict(X=odd), b"X must be 4-B aligned"), (dict(xy=None), b"xy and out"), (dict(out=None), b"xy and out"),
                    (dict(xy=odd), b"xy and out"), (dict(depth=odd), b"depth and alpha"), (dict(), b"null caps"),
                    (dict(depth=None, alpha=None), b"null caps")):
        assert call(**kw) == -1, kw
        assert msg in L.gwbp_last_error_string(), (kw, L.gwbp_last_error_string())


# ---- 5. the kernels' assembly --------------------------------------------------------------------------------------------------
def test_query_kernels_assembly(tmp_path):
    """Built for gfx950 at the product's flags: no scalar-unit instruction that writes memory (scalar stores, scalar atomics, scalar
    cache write-backs), no loop whose back edge is controlled by the exec mask (a lane-masked loop, the shape of the hang recorded in
    the README), no sleep-and-retry wait, no scratch, and the exact-fp32 matrix-core instruction only."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_asm_hazards
    flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
             "-fhip-fp32-correctly-rounded-divide-sqrt", "-munsafe-fp-atomics", "-fvisibility=hidden", "-S", "--cuda-device-only"]
    out = tmp_path / "query.s"
    subprocess.check_call([hipcc, *flags, "-o", str(out), os.path.join(_lib.CSRC, "query.hip")], stderr=subprocess.DEVNULL)
    assert check_asm_hazards.scan(str(out)) == []
    text = out.read_text()
    kernels = re.findall(r"^(_ZN4gwbp\S*k_(?:prompt_scores|probe_pixels)\S*):", text, flags=re.M)
    assert len(kernels) == 6, kernels  # scores: (aligned, element-wise) x (16, 32 prompts); probe: (aligned, element-wise)
    ops = [ln.split()[0] for ln in text.splitlines() if ln.startswith("\t") and not ln.startswith("\t.") and ln.split()]
    writes = [op for op in ops if op.startswith("s_") and (("st" + "ore") in op or "atomic" in op or ("dcache" in op and "inv" not in op))]
    assert writes == []
    assert not [op for op in ops if "atomic" in op]                      # bit-reproducible: no atomics of any kind
    assert not [ln for ln in text.splitlines() if "s_andn2_b64 exec, exec" in ln or "s_sleep" in ln]
    mfma = {op for op in ops if op.startswith("v_mfma")}
    assert mfma == {"v_mfma_f32_16x16x4_f32"}, mfma
    assert set(re.findall(r"\.private_segment_fixed_size: (\d+)", text)) == {"0"}
    assert set(re.findall(r"\.vgpr_spill_count: (\d+)", text)) == {"0"}
