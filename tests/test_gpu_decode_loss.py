"""gwbp_decode_loss and gsbp_amd.decoded_field on the GPU: the kernels alone against the float64 reference within the worst-case
rounding of their documented fp32 chains, every map form against the contiguous fp32 map bit for bit, reproducibility, memory,
the autograd path through rasterization() against the literal torch statement and against the oracle, and the fit loop.
Data, seeds and the reference: tests/decode_ref.py."""
import numpy as np
import pytest
import torch

import gsbp_amd
from gsbp_amd.rasterization import get_engine

import decode_ref as ref
import fidelity_ref as fid

pytestmark = pytest.mark.gpu
W, H, N = ref.W, ref.H, ref.N
U = ref.U
SHAPES = {0: (0, 7), 5: (1, 5), 64: (8, 8), 70 * 45: (45, 70)}  # P -> (H, W): empty, less than a block, one block, 50 slices
SCALE = 0.125


def engine(dev):
    return get_engine(dev, N, W, H)


def rows_per_slice(P):
    """The slice plan of include/gwbp.h: 64-pixel blocks, ceil(blocks / 512) blocks per slice."""
    nb = -(-P // 64)
    return 64 * max(1, -(-nb // 512))


def run(dev, R, C, M, hw, loss, **kw):
    h, w = hw
    d, D = C.shape
    out = engine(dev).decode_loss(torch.as_tensor(R).to(dev).reshape(h, w, d), torch.as_tensor(C).to(dev),
                                  torch.as_tensor(M).to(dev).reshape(h, w, D), loss=loss, scale=SCALE, **kw)
    return out


def assert_within_bounds(got, want, R, C, loss, what):
    """loss, GR, GC of one call against reference() within (n + 2) 2^-24 sum |terms|, n the chain length: d for y, D for GR, the
    slice's rows for GC's partials; for l2 the bound on g carries y's, to first order; l1's g is exact (no sign flips: l1_map)."""
    value, GR, GC, table = got
    P, d = R.shape
    D = C.shape[1]
    aR, aC = np.abs(R.astype(np.float64)), np.abs(C.astype(np.float64))
    by = (d + 2) * U * want["y_abs"]
    w = want["w"][:, None]
    if loss == "l1":
        dg = np.zeros_like(by)
        dterm = w * by + 2 * U * want["terms"]
    else:
        dg = 2 * w * by + 2 * U * np.abs(want["g"])
        dterm = w * 2 * np.abs(want["e"]) * by + 4 * U * want["terms"]
    dg, dterm = np.where(want["bad"][:, None], 0.0, dg), np.where(want["bad"][:, None], 0.0, dterm)
    b_gr = (D + 2) * U * (np.abs(want["g"]) @ aC.T) + dg @ aC.T
    b_gc = (rows_per_slice(P) + 2) * U * (aR.T @ np.abs(want["g"])) + aR.T @ dg
    b_loss = dterm.sum() + 18 * U * want["terms"].sum()  # + the 16-term fp32 sums of a lane
    for name, g_, w_, b_ in (("GR", GR.reshape(P, d), want["GR"], b_gr), ("GC", GC, want["GC"], b_gc)):
        err = np.abs(g_.double().cpu().numpy() - w_)
        worst = float((err / np.maximum(b_, 1e-300)).max()) if err.size else 0.0
        print(f"{what} {name}: max |err| = {float(err.max()) if err.size else 0.0:.3e}, max err / bound = {worst:.3f}")
        assert (err <= b_).all(), (what, name, worst)
    err = abs(float(value) - want["loss"])
    print(f"{what} loss: {float(value):.9e}, |err| = {err:.3e}, bound {b_loss:.3e}")
    assert err <= b_loss, (what, err, b_loss)
    t = table.cpu().numpy()
    assert t.tolist() == [float(value), P - want["n_bad"], want["n_bad"], P, d, D, 0.0, 0.0]


# ---- 1. the kernels alone -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["l1", "l2"])
@pytest.mark.parametrize("D", [16, 80, 512, 1040])
@pytest.mark.parametrize("d", [16, 48, 128])
@pytest.mark.parametrize("P", list(SHAPES))
def test_kernels_against_the_float64_reference(dev, P, d, D, loss):
    R, C, M = ref.kernel_inputs(P, d, D, seed=1, loss=loss)
    want = ref.reference(R, C, M, loss, SCALE)
    got = run(dev, R, C, M, SHAPES[P], loss)
    assert got[1].shape == (*SHAPES[P], d) and got[2].shape == (d, D) and got[0].dtype == torch.float64
    assert_within_bounds(got, want, R, C, loss, f"P={P} d={d} D={D} {loss}")


# ---- 2. map forms -------------------------------------------------------------------------------------------------------------------
def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("loss", ["l1", "l2"])
@pytest.mark.parametrize("d, D", [(48, 80), (128, 528)])
def test_map_forms_equal_the_contiguous_fp32_case_bit_for_bit(dev, d, D, loss):
    P, hw = 70 * 45, SHAPES[70 * 45]
    h, w = hw
    R, C, M = ref.kernel_inputs(P, d, D, seed=2, loss=loss)
    eng = engine(dev)
    r, c, m = torch.from_numpy(R).to(dev).reshape(h, w, d), torch.from_numpy(C).to(dev), torch.from_numpy(M).to(dev).reshape(h, w, D)
    kw = dict(loss=loss, scale=SCALE)
    base = eng.decode_loss(r, c, m, **kw)
    # half maps: the result on map.float(), and within the bounds of the reference on those values
    for dt in (torch.float16, torch.bfloat16):
        half = m.to(dt)
        got = eng.decode_loss(r, c, half, **kw)
        assert same(got, eng.decode_loss(r, c, half.float(), **kw)), dt
        if loss == "l2":  # (a rounded l1 map may move an error across zero: the l1 margin holds for the fp32 map only)
            want = ref.reference(R, C, half.float().cpu().numpy().reshape(P, D), loss, SCALE)
            assert_within_bounds(got, want, R, C, loss, str(dt))
    # strided and channel-padded maps, 16-B aligned or not; rendered rows and a decoder with padded strides
    for pad in (4, 3):
        wide = torch.zeros(h, w + 2, D + pad, device=dev)
        wide[:, :w, :D] = m
        assert same(eng.decode_loss(r, c, wide[:, :w, :D], **kw), base), pad
    rw = torch.zeros(h * w, d + 4, device=dev)
    rw[:, :d] = r.reshape(P, d)
    cw = torch.zeros(d, D + 3, device=dev)
    cw[:, :D] = c
    assert same(eng.decode_loss(rw[:, :d].unflatten(0, (h, w)), cw[:, :D], m, **kw), base)
    # GR written over R
    alias = r.clone()
    got = eng.decode_loss(alias, c, m, grad_rendered=alias, **kw)
    assert got[1].data_ptr() == alias.data_ptr() and same(got, base)
    # pixel weights: all ones (bool, fp32) change nothing; a bool mask equals its fp32 form and the reference
    for ones in (torch.ones(h, w, dtype=torch.bool, device=dev), torch.ones(h, w, device=dev)):
        assert same(eng.decode_loss(r, c, m, pixel_weights=ones, **kw), base), ones.dtype
    mask = torch.from_numpy(np.random.default_rng(8).uniform(size=(h, w)) < 0.7).to(dev)
    got = eng.decode_loss(r, c, m, pixel_weights=mask, **kw)
    assert same(got, eng.decode_loss(r, c, m, pixel_weights=mask.float(), **kw))
    assert same(got, eng.decode_loss(r, c, m, pixel_weights=mask.to(torch.float16), **kw))
    assert_within_bounds(got, ref.reference(R, C, M, loss, SCALE, mask.cpu().numpy().reshape(P)), R, C, loss, "mask")
    conf = torch.from_numpy(np.random.default_rng(9).uniform(0.0, 2.0, (h, w)).astype(np.float32)).to(dev)
    got = eng.decode_loss(r, c, m, pixel_weights=conf, **kw)
    # (the reference takes the kernel's w_p = fl(s c_p): SCALE is a power of two, the product is exact)
    assert_within_bounds(got, ref.reference(R, C, M, loss, SCALE, conf.cpu().numpy().reshape(P)), R, C, loss, "confidence")
    # one non-finite row (a NaN and an Inf in different chunks): every other GR row as before, its own zero; loss and GC are those
    # of the call that gives the pixel the weight zero, bit for bit
    bad = m.clone()
    bad[7, 33, 2], bad[7, 33, D - 1] = float("nan"), float("inf")
    got = eng.decode_loss(r, c, bad, **kw)
    zero_w = torch.ones(h, w, device=dev)
    zero_w[7, 33] = 0.0
    want = eng.decode_loss(r, c, m, pixel_weights=zero_w, **kw)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    assert not bool(got[1][7, 33].any()) and torch.equal(got[1][:7], base[1][:7]) and torch.equal(got[1][8:], base[1][8:])
    assert got[3].tolist()[1:4] == [P - 1, 1, P] and want[3].tolist()[1:4] == [P, 0, P]
    assert_within_bounds(got, ref.reference(R, C, bad.cpu().numpy().reshape(P, D), loss, SCALE), R, C, loss, "non-finite row")


# ---- 3. reproducibility and memory --------------------------------------------------------------------------------------------------
def test_two_runs_give_equal_bits(dev):
    for loss in ("l1", "l2"):
        R, C, M = ref.kernel_inputs(70 * 45, 128, 1040, seed=3, loss=loss)
        a, b = run(dev, R, C, M, SHAPES[70 * 45], loss), run(dev, R, C, M, SHAPES[70 * 45], loss)
        assert torch.equal(a[0].view(torch.int64), b[0].view(torch.int64)) and torch.equal(a[3].view(torch.int64), b[3].view(torch.int64))
        assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)) and torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))


def test_memory_beyond_the_outputs_does_not_depend_on_the_pixel_count(dev):
    d, D = 128, 512
    eng = engine(dev)
    rise = {}
    for P in (64, 70 * 45):
        h, w = SHAPES[P]
        R, C, M = ref.kernel_inputs(P, d, D, seed=4, loss="l2")
        r, c, m = torch.from_numpy(R).to(dev).reshape(h, w, d), torch.from_numpy(C).to(dev), torch.from_numpy(M).to(dev).reshape(h, w, D)
        gr = torch.empty_like(r)
        eng.decode_loss(r, c, m, loss="l2", grad_rendered=gr)  # (the workspace of (d, D) exists from here on)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.max_memory_allocated()
        out = eng.decode_loss(r, c, m, loss="l2", grad_rendered=gr)
        torch.cuda.synchronize()
        rise[P] = torch.cuda.max_memory_allocated() - before
        del out
    print(f"memory allocated during a call beyond grad_rendered: {rise}; one [P, D] fp32 image at P = 3150: {4 * 3150 * D}")
    assert rise[64] == rise[70 * 45] and rise[64] <= 4 * d * D + 1024


def test_argument_errors_raise_and_leave_the_device_usable(dev):
    eng = engine(dev)
    r, c, m = torch.zeros(8, 8, 16, device=dev), torch.zeros(16, 32, device=dev), torch.zeros(8, 8, 32, device=dev)
    for args, kw, msg in (((r[..., :8], c[:8], m), {}, "unsupported"), ((r, c[:, :24], m[..., :24]), {}, "unsupported"),
                          ((r, c, m[:4]), {}, "feature map"), ((r, c, m.double()), {}, "float32, float16 or bfloat16"),
                          ((r.cpu(), c, m), {}, "HIP tensor"), ((r, c, m), dict(loss="huber"), "loss"),
                          ((r, c, m), dict(grad_rendered=torch.zeros(8, 8, 8, device=dev)), "grad_rendered"),
                          ((r, c, m), dict(pixel_weights=torch.ones(4, 4, device=dev)), "pixel weights")):
        with pytest.raises(gsbp_amd.GwbpError, match=msg):
            eng.decode_loss(*args, **kw)
    value, gr, gc, table = eng.decode_loss(r, c, m)
    assert float(value) == 0.0 and not bool(gr.any()) and not bool(gc.any()) and table.tolist()[1:6] == [64, 0, 64, 16, 32]


# ---- 4. through rasterization() -----------------------------------------------------------------------------------------------------
_SCENE = {}


def scene(dev):
    if not _SCENE:
        gauss, vms, K = fid.scene()
        _SCENE.update(gauss=tuple(t.to(dev) for t in gauss), vms=vms.to(dev), K=K.to(dev))
    return _SCENE


@pytest.mark.parametrize("loss", ["l1", "l2"])
def test_autograd_path_against_the_literal_statement_and_the_oracle(dev, orc, loss):
    s = scene(dev)
    lat_h, conv_h, M_h, _ = ref.view_case()
    target = torch.from_numpy(M_h).to(dev)
    sens, live = ref.sensitive_gaussians(0, lat_h, conv_h, M_h, loss)
    assert (sens & live).sum() <= 0.01 * live.sum()  # before the kernel's output is looked at
    F = torch.nn.functional
    grads = {}
    for name in ("fused", "literal"):
        latents, conv = torch.from_numpy(lat_h).to(dev).requires_grad_(True), torch.from_numpy(conv_h).to(dev).requires_grad_(True)
        render, _, _ = gsbp_amd.rasterization(*s["gauss"], latents, s["vms"][:1], s["K"][None], W, H, want_meta=False)
        if name == "fused":
            value = gsbp_amd.decoded_loss(render, conv, target, loss=loss)
        else:
            value = (F.l1_loss if loss == "l1" else F.mse_loss)(render[0] @ conv, target)
        value.backward()
        grads[name] = (value.detach().double(), latents.grad.double(), conv.grad.double())
    for i, what in enumerate(("loss", "grad_latents", "grad_conv")):
        a, b = grads["fused"][i], grads["literal"][i]
        rel = float((a - b).abs().max() / b.abs().max())
        print(f"{loss} {what}: fused against literal, max |diff| / max |literal| = {rel:.3e}")
        assert rel <= ref.TOL, (what, rel)
    # the call without autograd: the same loss and decoder gradient bit for bit, the latent gradient through the same scatter
    out = gsbp_amd.decoded_field_gradients(*s["gauss"], torch.from_numpy(lat_h).to(dev), torch.from_numpy(conv_h).to(dev), target,
                                           s["vms"][0], s["K"], W, H, loss=loss)
    assert float(out["loss"].float()) == float(grads["fused"][0]) and torch.equal(out["grad_decoder"].double(), grads["fused"][2])
    diff = (out["grad_latents"].double() - grads["fused"][1]).abs().max() / grads["fused"][1].abs().max()
    assert float(diff) <= 1e-5, float(diff)  # (the scatter adds a Gaussian's tiles in no fixed order)
    assert out["table"].tolist()[1:6] == [H * W, 0, H * W, lat_h.shape[1], conv_h.shape[1]]
    # against the literal loop on the oracle's render, on the Gaussians that do not sit on a cut
    want = ref.literal_view(fid.pairs(0), lat_h, conv_h, M_h, loss)
    err = np.abs(out["grad_latents"].cpu().numpy() - want["grad_latents"])
    over = (err > ref.TOL * np.maximum(want["scale_latents"], 1e-30)).any(axis=1) & ~sens
    print(f"{loss}: {int(over.sum())} non-sensitive Gaussians beyond {ref.TOL} of their scale; {int((sens & live).sum())} sensitive")
    assert not over.any()
    assert abs(float(out["loss"]) - want["loss"]) <= ref.TOL * want["loss"]
    gc_err = np.abs(out["grad_decoder"].cpu().numpy() - want["grad_conv"]).max()
    assert gc_err <= ref.TOL * np.abs(want["grad_conv"]).max()


def test_second_order_use_falls_back_to_the_literal_expression(dev):
    r = torch.randn(4, 4, 16, device=dev, requires_grad=True)
    c = torch.rand(16, 32, device=dev, requires_grad=True)
    m = torch.randn(4, 4, 32, device=dev)
    (g,) = torch.autograd.grad(gsbp_amd.decoded_loss(r, c, m, loss="l2"), r, create_graph=True)
    (lit,) = torch.autograd.grad(torch.nn.functional.mse_loss(r @ c, m), r, create_graph=True)
    assert g.requires_grad and torch.allclose(g, lit, rtol=1e-5, atol=1e-8)
    (gg,) = torch.autograd.grad(g.square().sum(), c)
    (ll,) = torch.autograd.grad(lit.square().sum(), c)
    assert torch.allclose(gg, ll, rtol=1e-4, atol=1e-9)


# ---- 5. the fit ---------------------------------------------------------------------------------------------------------------------
def test_fit_follows_the_literal_loop_and_the_loss_falls(dev, orc):
    s = scene(dev)
    margin = ref.fit_margin()  # from the reference: 10 x the literal loop's float32 / float64 difference on the CPU
    maps = [torch.from_numpy(m).to(dev) for m in ref.fit_maps()]
    seen = []
    latents, decoder, history = gsbp_amd.fit_decoded_field(
        *s["gauss"], s["vms"], s["K"], W, H, lambda v: maps[v], ref.FIT_DIM, latent_dim=ref.FIT_RANK, steps=ref.FIT_STEPS,
        lr=ref.FIT_LR, loss="l2", seed=0, callback=lambda step, value, lat, dec: seen.append(step))
    assert latents.shape == (N, ref.FIT_RANK) and decoder.shape == (ref.FIT_RANK, ref.FIT_DIM) and seen == list(range(ref.FIT_STEPS))
    assert len(history) == ref.FIT_STEPS and history[-1] < history[0]
    # the literal torch loop on the device: same seeds, same Adam
    dec0, order = ref.fit_init(0)
    lat = torch.zeros(N, ref.FIT_RANK, device=dev, requires_grad=True)
    dec = dec0.to(dev).requires_grad_(True)
    opt = torch.optim.Adam([lat, dec], lr=ref.FIT_LR)
    literal = []
    for v in order:
        opt.zero_grad()
        render, _, _ = gsbp_amd.rasterization(*s["gauss"], lat, s["vms"][v:v + 1], s["K"][None], W, H, want_meta=False)
        value = torch.nn.functional.mse_loss(render[0] @ dec, maps[v])
        value.backward()
        opt.step()
        literal.append(float(value.detach()))
    rel = max(abs(a - b) / b for a, b in zip(history, literal))
    print(f"fit: loss {history[0]:.6e} -> {history[-1]:.6e}; largest per-step relative difference to the literal loop {rel:.3e}, "
          f"margin {margin:.3e} (recorded float32 / float64 figure {ref.FIT_F32_VS_F64:.1e})")
    assert rel <= margin
    # continuing from the result goes on from its loss
    _, _, more = gsbp_amd.fit_decoded_field(*s["gauss"], s["vms"], s["K"], W, H, lambda v: maps[v], ref.FIT_DIM, steps=2,
                                            lr=ref.FIT_LR, loss="l2", init=(latents, decoder), seed=1)
    assert max(more) < history[0]
    field = gsbp_amd.decode_field(latents, decoder)
    assert field.shape == (N, ref.FIT_DIM) and bool(torch.isfinite(field).all())
