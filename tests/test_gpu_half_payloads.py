"""fp16 / bf16 fields as render payloads, and half outputs, on the GPU.  The contract: a half payload gives the BITS the fp32 kernel
gives on payload.float(), NaN positions included, for every layout, and no fp32 copy of the payload is allocated; a half output is the
fp32 result rounded once, out32.to(dtype) bit for bit.

Scene: T1 (4 000 Gaussians, 200 x 136: both image sides end in a partial tile), view 0, one engine for every test.  Payload values are
drawn in fp32 and rounded to the half type; five Gaussians that do reach pixels of the view hold the special rows (zero, NaN, inf,
largest finite, subnormal).  Layouts: contiguous; row stride D + 4 (the packed loads where D allows them); row stride D + 1 on a view
that starts one element into its buffer (2-B aligned only: element loads), padding filled with NaN so that a read beyond D shows."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gsbp_amd
from gsbp_amd import sample, spatial, synthetic as syn

import half_fields_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF = (torch.float16, torch.bfloat16)
IDS = ["fp16", "bf16"]
LAYOUTS = ("contiguous", "stride D + 4", "stride D + 1, offset 1")
CFG = syn.CONFIGS["T1"]
N, W, H = CFG.n_gaussians, CFG.width, CFG.height
PX_DIMS = (1, 3, 4, 6, 16, 32)                 # k_render_px: every CH instantiation, odd strides
WIDE_DIMS = (17, 64, 130, 128, 260, 512, 516)  # k_render_rows below 128 and with D % 4 != 0 over two chunks; k_render_rows4 at Q = 1,
                                               # at Q = 2 and with a partial last block
CMP_DIMS = (6, 64, 260, 516)
_CTX = {}


def ctx(dev):
    """The scene on the device, an engine with view 0 projected, sorted and blended, and five Gaussians for the special rows: ones
    that hold weights in the view, but not the heaviest (a NaN row should not cover the image)."""
    if not _CTX:
        gauss = tuple(t.to(dev) for t in syn.activate(syn.make_scene(CFG)))
        vms, K = syn.make_cameras(CFG).to(dev), syn.intrinsics(CFG).to(dev)
        eng = gsbp_amd.Engine(N, W, H, device=dev)
        view = eng.view(vms[0], K, W, H)
        eng.project(view, *gauss)
        eng.bin_sort(view)
        eng.blend_weights(view)
        assert not eng.stats()["overflow"]
        counts = torch.bincount(eng.dump_pairs(view)[0].long(), minlength=N).cpu()
        seen = torch.nonzero(counts >= 4)[:, 0]
        assert seen.numel() >= 100
        order = seen[torch.argsort(counts[seen])]
        special = order[order.numel() // 2 - 2:order.numel() // 2 + 3]  # five around the median count
        g = torch.Generator().manual_seed(3)
        xy = torch.stack([torch.randint(0, W, (40,), generator=g), torch.randint(0, H, (40,), generator=g)], dim=1).to(torch.int32)
        xy[0], xy[1], xy[2] = torch.tensor([W - 1, H - 1]), torch.tensor([W, 3]), torch.tensor([-1, 0])  # the last pixel; two outside
        _CTX.update(gauss=gauss, vms=vms, K=K, eng=eng, view=view, special=special, xy=xy.to(dev))
    return _CTX


@functools.lru_cache(maxsize=None)
def _values(d: int, dtype) -> torch.Tensor:
    """[N, d] values drawn in fp32 and rounded to dtype, widened again, on the host; never modified.  (The special Gaussians are
    filled in by payload(): they depend on the view.)"""
    g = torch.Generator().manual_seed(1000 + d)
    return torch.randn(N, d, generator=g).to(dtype).float()


def payload32(dev, d: int, dtype) -> torch.Tensor:
    f = _values(d, dtype).clone()
    s = ctx(dev)["special"]
    f[s[0]] = 0.0
    f[s[1]] = float("nan")
    f[s[2]] = float("inf")
    if dtype == torch.float16:
        f[s[3], 0::2], f[s[3], 1::2] = 65504.0, -65504.0
        f[s[4]] = 2.0 ** -24  # the smallest fp16 subnormal
    else:
        f[s[3], 0::2], f[s[3], 1::2] = 3e38, -3e38
        f[s[4]] = 2.0 ** -130  # a bfloat16 subnormal
    h = f.to(dtype)
    assert bool((h[s[4]].float() > 0).all()) and bool(torch.isfinite(h[s[3]].float()).all())
    return h.float()


def layout(values32: torch.Tensor, dtype, how: str, dev) -> torch.Tensor:
    n, d = values32.shape
    if how == "contiguous":
        return values32.to(dtype).to(dev)
    if how == "stride D + 4":
        buf = torch.full((n, d + 4), float("nan"), dtype=dtype, device=dev)
        view = buf[:, :d]
    else:
        buf = torch.full((n * (d + 1) + 1,), float("nan"), dtype=dtype, device=dev)
        view = buf[1:].view(n, d + 1)[:, :d]
        assert view.data_ptr() % 4 == 2  # 2-B aligned only
    view.copy_(values32.to(dtype))
    return view


def _bits(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def same(a, b) -> bool:
    a, b = (a,) if torch.is_tensor(a) else tuple(a), (b,) if torch.is_tensor(b) else tuple(b)
    return len(a) == len(b) and all((x is None and y is None) or (x.dtype == y.dtype and x.shape == y.shape and
                                                                  torch.equal(_bits(x), _bits(y))) for x, y in zip(a, b))


def check_bits(call, dev, dims, dtype, what, needs_nan=True):
    """call(payload) on every layout of the half payload against the same call on payload.float(); a second run gives the same bits."""
    for d in dims:
        values = payload32(dev, d, dtype)
        want = call(values.to(dev))
        want_t = (want,) if torch.is_tensor(want) else tuple(t for t in want if t is not None)
        assert all(t.dtype != dtype for t in want_t)  # results keep their dtypes: nothing comes out in half
        if needs_nan:
            first = want_t[0]
            assert bool(torch.isnan(first).any()) and bool(torch.isfinite(first).any()), (what, d)  # the special rows are seen
        for how in LAYOUTS:
            f = layout(values, dtype, how, dev)
            assert f.dtype == dtype and torch.equal(_bits(f.float()), _bits(values))
            got = call(f)
            assert same(got, want), (what, d, how)
            assert same(call(f), got), (what, d, how, "second run")


# ---- bits: the four Engine calls ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", HALF, ids=IDS)
def test_render_pixels_of_a_half_table(dev, dtype):
    c = ctx(dev)
    check_bits(lambda f: c["eng"].render_pixels(c["view"], f, want_alphas=True), dev, PX_DIMS, dtype, "render_pixels")


@pytest.mark.parametrize("dtype", HALF, ids=IDS)
def test_wide_render_of_a_half_table(dev, dtype):
    c = ctx(dev)
    check_bits(lambda f: c["eng"].render(c["view"], f), dev, WIDE_DIMS, dtype, "render")


@pytest.mark.parametrize("dtype", HALF, ids=IDS)
def test_probe_of_a_half_table(dev, dtype):
    c = ctx(dev)
    check_bits(lambda f: c["eng"].probe_pixels(c["view"], c["xy"], f), dev, WIDE_DIMS, dtype, "probe_pixels", needs_nan=False)
    # the probe is the render at those pixels: the half table through one kernel against the fp32 table through the other
    f = payload32(dev, 130, dtype)
    out = c["eng"].probe_pixels(c["view"], c["xy"], layout(f, dtype, LAYOUTS[2], dev))[0]
    img = c["eng"].render(c["view"], f.to(dev))
    inside = (c["xy"][:, 0] >= 0) & (c["xy"][:, 0] < W) & (c["xy"][:, 1] >= 0) & (c["xy"][:, 1] < H)
    xy = c["xy"][inside].long()
    assert same(out[inside], img[xy[:, 1], xy[:, 0]]) and not bool(out[~inside].any())


@pytest.mark.parametrize("map_half", (False, True), ids=["fp32 map", "half map"])
@pytest.mark.parametrize("dtype", HALF, ids=IDS)
def test_field_compare_of_a_half_field(dev, dtype, map_half):
    c = ctx(dev)
    for d in CMP_DIMS:
        fmap = syn.make_feature_map(CFG, 0, device=dev, dim=d)
        if map_half:
            fmap = fmap.to(dtype)
        check_bits(lambda f: c["eng"].field_compare(c["view"], f, fmap), dev, (d,), dtype, "field_compare")  # (planes, table)
    # the table alone, into a row of the caller's
    f = payload32(dev, 64, dtype)
    rows = torch.zeros(2, 8, dtype=torch.float64, device=dev)
    fmap = syn.make_feature_map(CFG, 0, device=dev, dim=64)
    planes, table = c["eng"].field_compare(c["view"], layout(f, dtype, LAYOUTS[1], dev), fmap, want_planes=False, table=rows[1])
    assert planes is None and same(table, c["eng"].field_compare(c["view"], f.to(dev), fmap)[1]) and not bool(rows[0].any())


# ---- bits: the public functions ------------------------------------------------------------------------------------------------------
def _public(dev):
    c = ctx(dev)
    g, vm, K = c["gauss"], c["vms"][0], c["K"]
    fmaps = {}

    def fmap(d):
        if d not in fmaps:
            fmaps[d] = syn.make_feature_map(CFG, 0, device=dev, dim=d)
        return fmaps[d]

    def agreement(f):
        out = gsbp_amd.render_field_agreement(*g, f, fmap(f.shape[1]), vm, K, W, H)
        return tuple(out[k] for k in ("dot", "rr", "mm", "l1", "l2", "cosine", "alpha"))

    return {
        "rasterization": lambda f: gsbp_amd.rasterization(*g, f, c["vms"][:1], K[None], W, H, want_meta=False)[:2],
        "probe_pixels": lambda f: gsbp_amd.probe_pixels(*g, f, vm, K, W, H, c["xy"]),
        "render_field_agreement": agreement,
        "score_field_views": lambda f: gsbp_amd.score_field_views(*g, f, c["vms"], K, W, H, lambda v: fmap(f.shape[1]) if v == 0 else None),
    }


PUBLIC = ("rasterization", "probe_pixels", "render_field_agreement", "score_field_views")


@pytest.mark.parametrize("dtype", HALF, ids=IDS)
@pytest.mark.parametrize("name", PUBLIC)
def test_public_functions_take_a_half_field(dev, name, dtype):
    check_bits(_public(dev)[name], dev, (16, 64), dtype, name, needs_nan=name in ("rasterization", "render_field_agreement"))


@pytest.mark.parametrize("dtype", HALF, ids=IDS)
@pytest.mark.parametrize("name", PUBLIC)
def test_public_functions_read_a_half_field_without_a_second_field(dev, name, dtype):
    """test_half_field_is_read_without_a_second_field's criterion and warm-up (test_gpu_half_fields.py): the allocator's peak over the
    call on the half field is at most its peak over the same call on an fp32 field made beforehand; a copy would add 4 N D = 8 MB."""
    d = 512
    call = _public(dev)[name]
    g = torch.Generator().manual_seed(5)
    f32 = torch.nn.functional.normalize(torch.randn(N, d, generator=g), dim=1).to(dtype).float().to(dev)
    f16 = f32.to(dtype)
    peaks = []
    for f in (f32, f16):
        call(f)  # (warm: the library, the allocator's pools, the engine and its front cache)
        torch.cuda.synchronize(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        call(f)
        torch.cuda.synchronize(dev)
        peaks.append(torch.cuda.max_memory_allocated(dev))
    print(f"{name} {dtype}: peak {peaks[0]} B on fp32, {peaks[1]} B on half, a copy would add {4 * N * d} B")
    assert peaks[1] <= peaks[0], (name, peaks, 4 * N * d)


# ---- half outputs --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lists(n_rows: int, n_src: int, k: int = 5):
    g = torch.Generator().manual_seed(77)
    idx = torch.randint(0, n_src, (n_rows, k), generator=g, dtype=torch.int32)
    idx[torch.rand(n_rows, k, generator=g) < 0.15] = -1
    idx[7] = -1  # a row without a neighbour
    w = torch.rand(n_rows, k, generator=g)
    w[torch.rand(n_rows, k, generator=g) < 0.1] = 0.0
    return idx, w


@pytest.mark.parametrize("dtype", HALF, ids=IDS)
def test_half_outputs_are_the_fp32_results_rounded_once(dev, dtype):
    c = ctx(dev)
    n = 300
    idx, w = (t.to(dev) for t in _lists(n, n))
    means = c["gauss"][0][:n].contiguous()
    for d in (1, 6, 64, 260, 516):
        v = payload32(dev, d, dtype)[:n] * 3.0
        v[:, 1::3] *= 1e-6  # fp16 subnormals beside entries of order 1 ...
        v[:, 2::5] *= 1e-9  # ... and results that underflow to zero
        for src in (v.to(dev), layout(v.to(dtype).float(), dtype, LAYOUTS[2], dev)):  # an fp32 field; a half one, element loads
            calls = {
                "neighbor_mean": lambda od: spatial.neighbor_mean(src, idx, out_dtype=od),
                "neighbor_blend": lambda od: sample.neighbor_blend(src, idx, w, out_dtype=od)[0],
                "smooth_features": lambda od: gsbp_amd.smooth_features(means, src, k=6, out_dtype=od),
            }
            for name, call in calls.items():
                full = call(None)
                assert full.dtype == torch.float32 and same(full, call(torch.float32)), name  # the default is what it was
                half = call(dtype)
                assert half.dtype == dtype and half.shape == full.shape and half.is_contiguous()
                assert same(half, full.to(dtype)), (name, d, src.dtype)
    for d in WIDE_DIMS:  # the render's epilogues: both kernels, every chunk form
        for f in (payload32(dev, d, dtype).to(dev), layout(payload32(dev, d, dtype), dtype, LAYOUTS[0], dev)):
            full = c["eng"].render(c["view"], f)
            assert full.dtype == torch.float32 and same(full, c["eng"].render(c["view"], f, out_dtype=torch.float32))
            half = c["eng"].render(c["view"], f, out_dtype=dtype)
            assert half.dtype == dtype and same(half, full.to(dtype)), (d, f.dtype)
    with pytest.raises(gsbp_amd.GwbpError):
        spatial.neighbor_mean(v.to(dev), idx, out_dtype=torch.float64)
    with pytest.raises(gsbp_amd.GwbpError):
        c["eng"].render(c["view"], f, out_dtype=torch.float64)


@pytest.mark.parametrize("dtype", HALF, ids=IDS)
def test_sample_field_writes_out_dtype_with_both_fallbacks(dev, dtype):
    c = ctx(dev)
    pts = sample.synthetic_points(c["gauss"][0], count=512)
    pg = gsbp_amd.point_gaussians(pts, *c["gauss"], k=8)
    for f in (payload32(dev, 36, dtype).to(dev), payload32(dev, 36, dtype).to(dtype).to(dev)):
        for fallback in ("none", "nearest"):
            full, valid = gsbp_amd.sample_field(f, pg, fallback=fallback)
            assert full.dtype == torch.float32 and bool((~valid).any()) and bool(valid.any())
            half, valid_h, wsum = gsbp_amd.sample_field(f, pg, fallback=fallback, out_dtype=dtype, return_wsum=True)
            assert half.dtype == dtype and wsum.dtype == torch.float32 and torch.equal(valid_h, valid)
            assert same(half, full.to(dtype)), (fallback, f.dtype)
        assert bool(full[~valid].any())  # the "nearest" fallback did fill rows
    moved, valid, _ = gsbp_amd.transfer_field(*c["gauss"], f, pts, out_dtype=dtype)
    assert moved.dtype == dtype and moved.shape == (pts.shape[0], 36)


@pytest.mark.parametrize("dtype,bits,ties", [(torch.float16, ref.f32_to_f16_bits, ref.F16_TIES),
                                             (torch.bfloat16, ref.f32_to_bf16_bits, ref.BF16_TIES)], ids=IDS)
def test_one_neighbour_of_weight_one_passes_rows_through_the_rounding(dev, dtype, bits, ties):
    """x / 1 and fmaf(1, x, 0) / 1 are x: the stored half is the rounding of the row itself, checked against the integer-arithmetic
    references on exact ties, fp16 subnormals and values that underflow."""
    g = torch.Generator().manual_seed(99)
    n, d = 96, 23
    x = torch.randn(n, d, generator=g)
    x[:, 1::3] *= 1e-6
    x[:, 2::5] *= 1e-9
    for i, m in enumerate(ties):
        x[3 + 2 * i] = torch.from_numpy(ref.tie_row(m, d))
        x[4 + 2 * i] = -x[3 + 2 * i]
    x[x == 0] = 0.0  # (+0 + -0 is +0: a sum does not keep the sign of a zero)
    want = bits(x.numpy())
    idx = torch.arange(n, dtype=torch.int32, device=dev)[:, None].contiguous()
    ones = torch.ones(n, 1, device=dev)
    for got in (spatial.neighbor_mean(x.to(dev), idx, out_dtype=dtype), sample.neighbor_blend(x.to(dev), idx, ones, out_dtype=dtype)[0]):
        assert got.dtype == dtype and np.array_equal(got.cpu().view(torch.int16).numpy().view(np.uint16), want)
    for i, m in enumerate(ties):  # the ties do round to even
        step = 2 if dtype == torch.float16 else 16
        lo = m // step * step
        even = lo if (lo // step) % 2 == 0 else lo + step
        assert float(got[3 + 2 * i, 0]) == even * 2.0 ** -12 and float(got[4 + 2 * i, 0]) == -even * 2.0 ** -12
    if dtype == torch.float16:
        mag = x.abs()
        assert bool(((mag > 0) & (mag < 2.0 ** -25)).any()) and bool(((mag > 2.0 ** -24) & (mag < 2.0 ** -14)).any())


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    c = ctx(dev)
    g, K = c["gauss"], c["K"]
    for dtype in HALF:
        colors = torch.rand(N, 16, device=dev).to(dtype).requires_grad_(True)
        with pytest.raises(NotImplementedError):
            gsbp_amd.rasterization(*g, colors, c["vms"][:1], K[None], W, H)
    f64 = torch.rand(N, 16, device=dev, dtype=torch.float64)
    with pytest.raises(gsbp_amd.GwbpError):
        gsbp_amd.rasterization(*g, f64, c["vms"][:1], K[None], W, H)
    for call in (lambda: c["eng"].render(c["view"], f64), lambda: c["eng"].render_pixels(c["view"], f64),
                 lambda: c["eng"].probe_pixels(c["view"], c["xy"], f64),
                 lambda: c["eng"].field_compare(c["view"], f64, syn.make_feature_map(CFG, 0, device=dev, dim=16)),
                 lambda: gsbp_amd.probe_pixels(*g, f64, c["vms"][0], K, W, H, c["xy"])):
        with pytest.raises(gsbp_amd.GwbpError):
            call()


# ---- the command lines ---------------------------------------------------------------------------------------------------------------
def test_cli_smooths_into_bf16_and_clicks_on_a_bf16_field(tmp_path, dev):
    def run(script, *argv):
        r = subprocess.run([sys.executable, os.path.join(ROOT, script), *argv], capture_output=True, text=True)
        assert r.returncode == 0, (script, r.stderr[-2000:])

    cfg = syn.CONFIGS["C1"]
    g = torch.Generator().manual_seed(21)
    field = torch.nn.functional.normalize(torch.randn(cfg.n_gaussians, cfg.feat_dim, generator=g), dim=1).to(torch.bfloat16)
    half_path, full_path = str(tmp_path / "field_bf16.pt"), str(tmp_path / "field_f32.pt")
    torch.save(field, half_path)
    torch.save(field.float(), full_path)
    clean = str(tmp_path / "clean")
    run("run_clean.py", "--synthetic", "C1", "--features", half_path, "--field-dtype", "bf16", "--out", clean)
    smoothed = torch.load(os.path.join(clean, "features.pt"))
    assert smoothed.dtype == torch.bfloat16 and smoothed.shape == field.shape and bool(torch.isfinite(smoothed.float()).all())
    masks = []
    for name, path in (("half", half_path), ("full", full_path)):
        out = str(tmp_path / f"segment_{name}")
        run("run_segment.py", "--synthetic", "C1", "--features", path, "--click", f"0:{cfg.width // 2},{cfg.height // 2}",
            "--max-views", "1", "--out", out)
        masks.append(torch.load(os.path.join(out, "mask3d.pt")))
    assert masks[0].dtype == torch.bool and masks[0].shape == (cfg.n_gaussians,) and torch.equal(masks[0], masks[1])
