"""fp16 / bf16 feature maps on the GPU: every path that reads them natively (the 256- and the 128-channel scatter kernel at full
resolution, nearest-index and bilinear; token space) must give what the fp32 path gives on map.float() -- up to the order of the
atomic sums, bit for bit in token space -- and the paths that widen the map at the call must give exactly that too."""
import numpy as np
import pytest
import torch

from util import rel_row_err, scene_np, to_dev

import gsbp_amd
from gsbp_amd import synthetic as syn

pytestmark = pytest.mark.gpu

HALF = [torch.float16, torch.bfloat16]
N_CLASS = 5  # channel c holds values of class c % 5, see _special_map


def _special_map(h, w, D, dtype, dev, seed=0):
    """[h, w, D] map of `dtype` whose channels cycle through five value classes: 0 ordinary N(0, 1); 1 tiny values (fp16
    subnormals, 2^-24 .. 2^-15); 2 signed zeros; 3 magnitudes near the fp16 maximum (57344 .. 65504); 4 1 + k 2^-7 with k odd (bf16
    values whose lowest mantissa bit is set).  A kernel that reads fp16 bits as bf16, flushes subnormals, drops the sign of a
    zero or truncates a mantissa gets at least one class visibly wrong."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    sign = torch.where(torch.rand(h, w, D, generator=g) < 0.5, -1.0, 1.0)
    cls = torch.arange(D) % N_CLASS
    ordinary = torch.randn(h, w, D, generator=g)
    tiny = torch.randint(1, 512, (h, w, D), generator=g).float() * 2.0 ** -24
    big = 57344.0 + torch.randint(0, 256, (h, w, D), generator=g).float() * 32.0
    lowbit = 1.0 + (2 * torch.randint(0, 64, (h, w, D), generator=g) + 1).float() * 2.0 ** -7
    v = torch.where(cls == 0, ordinary, torch.where(cls == 1, tiny * sign, torch.where(cls == 2, 0.0 * sign,
                    torch.where(cls == 3, big * sign, lowbit * sign))))
    return v.to(dtype).to(dev)


def _check_classes(F, Fr, tol=1e-5):
    """rel_row_err per value class (a row's norm is dominated by the near-maximum class otherwise)."""
    F, Fr = F.cpu().numpy(), Fr.cpu().numpy()
    for c in range(N_CLASS):
        if c == 2:  # signed zeros: nothing may leak in
            assert not F[:, c::N_CLASS].any() and not Fr[:, c::N_CLASS].any()
            continue
        assert np.abs(Fr[:, c::N_CLASS]).max() > 0, c
        assert rel_row_err(F[:, c::N_CLASS], Fr[:, c::N_CLASS]) <= tol, c


@pytest.fixture(scope="module")
def t1(dev):
    cfg, sc = scene_np("T1")
    return cfg, to_dev(sc, dev)


def _weighted(eng, cfg, g, feats, dev, upsample=None):
    """project + sort + blend of view 0, then scatter of `feats`: F, d, counters."""
    view = eng.view(g["vms"][0], g["K"], cfg.width, cfg.height)
    eng.project(view, g["means"], g["quats"], g["scales"], g["opac"])
    eng.bin_sort(view)
    eng.blend_weights(view)
    F = torch.zeros(cfg.n_gaussians, feats.shape[2], device=dev)
    d = torch.zeros(cfg.n_gaussians, device=dev)
    eng.scatter(view, feats, F, d, upsample=upsample)
    st = eng.stats()
    assert st["overflow"] == 0
    return F, d, st


@pytest.mark.parametrize("dtype", HALF, ids=["f16", "bf16"])
@pytest.mark.parametrize("upsample", [None, "nearest", "bilinear"], ids=["full", "nearest", "bilinear"])
@pytest.mark.parametrize("D,narrow", [(512, False), (384, False), (512, True)], ids=["wide512", "full384", "full512narrow"])
def test_native_scatter_matches_fp32_on_the_widened_map(t1, dev, dtype, upsample, D, narrow):
    cfg, g = t1
    h, w = (cfg.height, cfg.width) if upsample is None else (23, 37)
    m = _special_map(h, w, D, dtype, dev, seed=D + 7 * (upsample is None))
    eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev)
    eng.set_narrow_scatter(narrow)
    assert eng.half_native(m)  # the typed entry point, not a conversion
    F, d, st = _weighted(eng, cfg, g, m, dev, upsample)
    Fr, dr, sr = _weighted(eng, cfg, g, m.float(), dev, upsample)
    _check_classes(F, Fr)
    assert rel_row_err(d.cpu().numpy()[:, None], dr.cpu().numpy()[:, None]) <= 1e-5
    assert st["n_pairs"] == sr["n_pairs"] and st["n_headers"] == sr["n_headers"] and st["n_pairs"] > 0


@pytest.mark.parametrize("dtype", HALF, ids=["f16", "bf16"])
@pytest.mark.parametrize("D", [1024, 384])
def test_token_space_is_bit_identical_to_fp32_tokens(t1, dev, dtype, D):
    cfg, g = t1
    tok = _special_map(8, 12, D, dtype, dev, seed=D)
    eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev)
    assert eng.can_scatter_tokens(tok, cfg.height, cfg.width)
    out = []
    for t in (tok, tok.float()):
        view = eng.view(g["vms"][0], g["K"], cfg.width, cfg.height)
        eng.project(view, g["means"], g["quats"], g["scales"], g["opac"])
        eng.bin_sort(view)
        eng.blend_tokens(view, 8, 12)
        F = torch.zeros(cfg.n_gaussians, D, device=dev)
        d = torch.zeros(cfg.n_gaussians, device=dev)
        eng.scatter_tokens(view, t, F, d, scale_f=0.5, scale_d=2.0)
        assert eng.stats()["overflow"] == 0
        out.append((F, d))
    assert float(out[1][0].abs().max()) > 0
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


@pytest.mark.parametrize("dtype", HALF, ids=["f16", "bf16"])
def test_conversion_paths_equal_fp32(t1, dev, dtype):
    """Maps no native kernel takes are widened at the call: D = 32 (the fused blend + scatter), the encoder-fused scatter and a
    channel-major (non-contiguous) map."""
    cfg, g = t1
    eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev)
    m32 = _special_map(cfg.height, cfg.width, 32, dtype, dev, seed=1)
    assert not eng.half_native(m32)
    F, _, st = _weighted(eng, cfg, g, m32, dev)
    Fr, _, sr = _weighted(eng, cfg, g, m32.float(), dev)
    _check_classes(F, Fr)
    assert st["n_pairs"] == sr["n_pairs"]
    # channel-major [D, H, W] storage seen as [H, W, D]: fs_c != 1
    cm = _special_map(cfg.height, cfg.width, 128, dtype, dev, seed=2).permute(2, 0, 1).contiguous().permute(1, 2, 0)
    assert cm.stride(2) != 1 and not eng.half_native(cm)
    F, _, _ = _weighted(eng, cfg, g, cm, dev)
    Fr, _, _ = _weighted(eng, cfg, g, cm.float(), dev)
    _check_classes(F, Fr)
    # encoder fused into the staging: [H, W, 64] @ [64, 16]
    gen = torch.Generator(device="cpu").manual_seed(3)
    enc = torch.randn(64, 16, generator=gen).to(dev)
    mk = (torch.randn(cfg.height, cfg.width, 64, generator=gen) * 4).to(dtype).to(dev)
    assert eng.can_fuse_encoder(mk, enc)
    res = []
    for t in (mk, mk.float()):
        view = eng.view(g["vms"][0], g["K"], cfg.width, cfg.height)
        eng.project(view, g["means"], g["quats"], g["scales"], g["opac"])
        eng.bin_sort(view)
        eng.blend_weights(view)
        F = torch.zeros(cfg.n_gaussians, 16, device=dev)
        d = torch.zeros(cfg.n_gaussians, device=dev)
        eng.scatter_encoded(view, t, enc, F, d)
        res.append(F.cpu().numpy())
    assert np.abs(res[1]).max() > 0 and rel_row_err(res[0], res[1]) <= 1e-5


@pytest.mark.parametrize("pipeline", [True, False], ids=["pipelined", "serial"])
@pytest.mark.parametrize("dtype", HALF, ids=["f16", "bf16"])
def test_create_feature_field_with_a_half_feature_fn(dev, dtype, pipeline):
    cfg, sc = scene_np("T1")
    g = to_dev(sc, dev)
    D, V = 512, 2
    maps = [_special_map(cfg.height, cfg.width, D, dtype, dev, seed=40 + v) for v in range(V)]
    args = (g["means"], g["quats"], g["scales"], g["opac"], g["vms"][:V], g["K"], cfg.width, cfg.height)
    _, F, d, st = gsbp_amd.create_feature_field(*args, lambda v: maps[v], D, return_partials=True, pipeline=pipeline)
    _, Fr, dr, sr = gsbp_amd.create_feature_field(*args, lambda v: maps[v].float(), D, return_partials=True, pipeline=pipeline)
    assert st["overflow"] == 0 and st["n_pairs"] == sr["n_pairs"] and st["n_headers"] == sr["n_headers"]
    _check_classes(F, Fr)
    assert rel_row_err(d.cpu().numpy()[:, None], dr.cpu().numpy()[:, None]) <= 1e-5


@pytest.mark.parametrize("dtype", HALF, ids=["f16", "bf16"])
def test_c2_view_against_the_oracle_fed_the_widened_map(dev, orc, dtype):
    """One full-size C2 view (1M Gaussians, 1600 x 1060, D = 512: the 256-channel kernel) through create_feature_field with a half
    map, against the CPU oracle fed map.float()."""
    cfg = syn.CONFIGS["C2"]
    D = cfg.feat_dim
    g_cpu = syn.activate(syn.make_scene(cfg))
    g = [t.to(dev) for t in g_cpu]
    vms, K = syn.make_cameras(cfg, n_views=1), syn.intrinsics(cfg)
    m = syn.make_feature_map(cfg, 30, device=dev).to(dtype)
    out, F, d, st = gsbp_amd.create_feature_field(*g, vms.to(dev), K.to(dev), cfg.width, cfg.height, lambda v: m, D,
                                                  return_partials=True)
    assert st["overflow"] == 0
    h = [t.numpy() for t in g_cpu]
    Fr = np.zeros((cfg.n_gaussians, D), np.float32)
    dr = np.zeros(cfg.n_gaussians, np.float32)
    info = orc.backproject_view(*h, vms[0].numpy(), K.numpy(), cfg.width, cfg.height, m.float().cpu().numpy(), Fr, dr)
    assert st["n_pairs"] == info["n_pairs"]
    assert rel_row_err(F.cpu().numpy(), Fr) <= 1e-4
    assert rel_row_err(d.cpu().numpy()[:, None], dr[:, None]) <= 1e-4
