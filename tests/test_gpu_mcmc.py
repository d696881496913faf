"""The MCMC strategy on the GPU (csrc/mcmc.hip): every kernel against tests/mcmc_ref.py bit for bit -- with the
device's own expf, logf and powf handed to the restatement (gwbp_mcmc_libm), each of them held to its documented error against
float64 -- at the wave, block and block-carry edges of the scan; the rounds with an Adam optimiser and carried tables; determinism; the
statistics of the draws and of the noise on the seeds tests/test_mcmc_cpu.py verified against the reference; train_scene under the
strategy on T0; and what a kernel does with arguments the host cannot check.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import mcmc_ref as ref
import gsbp_amd
from gsbp_amd import _lib, mcmc
from gsbp_amd._lib import ptr
from test_gpu_densify import t0_training_setup
from test_mcmc_cpu import (MIN_OPACITY, check_noise_variance, check_sampling, heavy_scene, noise_rows, noise_variance_case, same_bits,
                           sampling_case, scene, sorted_u)

pytestmark = pytest.mark.gpu
T_OPA = float(np.float32(ref.logit(float(np.float32(MIN_OPACITY)))))


class DeviceLib:
    """expf, logf and powf as the kernels evaluate them."""

    def __init__(self, dev):
        self.dev = dev

    def _run(self, op, a, b=None):
        a = ref.f32(a)
        tb = None if b is None else torch.from_numpy(np.array(np.broadcast_to(b, a.shape), dtype=np.float32)).to(self.dev)
        return mcmc.device_libm(op, torch.from_numpy(a).to(self.dev), tb).cpu().numpy()

    def exp(self, a):
        return self._run("exp", a)

    def log(self, a):
        return self._run("log", a)

    def pow(self, a, b):
        return self._run("pow", a, b)


def up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def test_the_device_library_calls_within_their_documented_error(dev):
    """The device library is built to OpenCL's error table: exp and log within 3 units in the last place, pow within 16."""
    r = np.random.default_rng(2)
    lib = DeviceLib(dev)
    a, p = ref.f32(r.uniform(-20.0, 20.0, 50000)), ref.f32(r.uniform(1e-6, 1.0, 50000))
    e = ref.f32(1.0 / r.integers(1, 52, 50000))
    worst = {}
    for name, got, want, limit in (("exp", lib.exp(a), np.exp(a.astype(np.float64)), 3.0), ("log", lib.log(p), np.log(p.astype(np.float64)), 3.0),
                                   ("pow", lib.pow(p, e), np.power(p.astype(np.float64), e.astype(np.float64)), 16.0)):
        ulp = np.abs(got.astype(np.float64) - want) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        worst[name] = float(ulp.max())
        assert ulp.max() <= limit, (name, ulp.max())
    print(f"device expf, logf, powf against float64, in units in the last place: {worst}")


# ---- plan, draw, update against the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 65536, 65537])
def test_plan_draw_update_bit_for_bit(dev, n):
    lib = DeviceLib(dev)
    t = scene(max(n, 8), seed=5 + n % 7)
    t = {k: v[:n].copy() for k, v in t.items()}
    if n == 1:
        t["opacity"][0] = 0.5
    opacity = up(t["opacity"], dev)
    for mode, code in (("relocate", ref.RELOCATE), ("add", ref.ADD)):
        cdf, dead_offsets, dead_idx = mcmc.plan(opacity, T_OPA, mode)
        want_cdf, want_off, want_idx = ref.plan(t["opacity"], T_OPA, code, lib)
        assert np.array_equal(cdf.cpu().numpy(), want_cdf) and np.array_equal(dead_offsets.cpu().numpy(), want_off), mode
        assert np.array_equal(dead_idx.cpu().numpy()[:len(want_idx)], want_idx), mode
        if n >= 255:
            assert 0 < len(want_idx) < n and {0, n - 1, n // 2} <= set(want_idx.tolist())  # the first and the last row and the NaN are dead
        for m in sorted({0, 1, n, 3 * n}):
            u = sorted_u(m, 17 + m % 5)
            parent = mcmc.draw(cdf, up(u, dev))
            want_parent = ref.draw(want_cdf, u) if n > 0 else np.full(m, -1, np.int32)
            assert np.array_equal(parent.cpu().numpy(), want_parent), (mode, m)
            if n == 0:
                continue
            o, s = opacity.clone(), up(t["scaling"], dev)
            count = mcmc.update(o, s, parent, MIN_OPACITY)
            want_o, want_s, want_count = ref.update(t["opacity"], t["scaling"], want_parent, MIN_OPACITY, lib)
            assert np.array_equal(count.cpu().numpy(), want_count), (mode, m)
            fin = np.isfinite(want_o) & np.isfinite(want_s).all(axis=1)
            assert fin.sum() >= n - 2
            assert same_bits(o.cpu().numpy()[fin], want_o[fin]) and same_bits(s.cpu().numpy()[fin], want_s[fin]), (mode, m)
            if mode == "relocate" and m > 0:
                assert want_count[want_idx].sum() == 0  # a dead Gaussian is never a parent


def test_a_parent_drawn_sixty_times_clamps_at_ratio_51(dev):
    lib = DeviceLib(dev)
    t = heavy_scene()
    n = len(t["opacity"])
    cdf, dead_offsets, dead_idx = mcmc.plan(up(t["opacity"], dev), T_OPA, "relocate")
    m = int(dead_offsets[n])
    u = sorted_u(n, 3)[:m]
    parent = mcmc.draw(cdf, up(u, dev))
    o, s = up(t["opacity"], dev), up(t["scaling"], dev)
    count = mcmc.update(o, s, parent, MIN_OPACITY).cpu().numpy()
    want_o, want_s, want_count = ref.update(t["opacity"], t["scaling"], ref.draw(ref.plan(t["opacity"], T_OPA, lib=lib)[0], u), MIN_OPACITY, lib)
    assert count.max() >= 60 and np.array_equal(count, want_count)
    assert same_bits(o.cpu().numpy(), want_o) and same_bits(s.cpu().numpy(), want_s)
    # ... and the device's values lie inside the bound the float64 literal rule is held to, with the device library's error in place of
    # one unit: the bound charges 2 u per call, the device may take 16 (pow) -- it does not need them
    hit = np.nonzero(count)[0]
    b_logit, b_s = ref.relocation_bounds(t["opacity"][hit], t["scaling"][hit], np.minimum(count[hit] + 1, 51), MIN_OPACITY)
    lit, _, _, _ = ref.literal_relocate(t, {}, MIN_OPACITY, parent.cpu().numpy())
    worst = max(float((np.abs(o.cpu().numpy()[hit] - lit["opacity"][hit]) / b_logit).max()),
                float((np.abs(s.cpu().numpy()[hit] - lit["scaling"][hit]) / b_s).max()))
    print(f"device o' and s' against the float64 literal rule: largest error / bound = {worst:.3f}")
    assert worst < 1.0


@pytest.mark.parametrize("case", ["all_dead", "none_dead"])
def test_rounds_that_do_nothing(dev, case):
    t = scene(300, seed=4)
    t["opacity"][:] = -9.0 if case == "all_dead" else np.abs(t["opacity"]) - 5.0
    if case == "none_dead":
        t["opacity"] = np.nan_to_num(t["opacity"], nan=0.0)
    splats = {k: up(v, dev) for k, v in t.items() if k != "field"}
    before = {k: v.clone() for k, v in splats.items()}
    out, info = gsbp_amd.relocate(splats, gsbp_amd.MCMCConfig(), generator=torch.Generator(device=dev).manual_seed(1))
    assert out is splats and info["relocated"] == 0 and info["parent"] is None
    assert (info["n_dead"], info["total_weight"] == 0) == ((300, True) if case == "all_dead" else (0, False))
    assert all(torch.equal(splats[k], before[k]) for k in splats)
    if case == "all_dead":  # total weight 0: every draw answers -1, and nothing downstream writes
        cdf, _, dead_idx = mcmc.plan(splats["opacity"], T_OPA, "relocate")
        parent = mcmc.draw(cdf, up(sorted_u(300, 1), dev))
        assert bool((parent == -1).all())
        assert not mcmc.update(splats["opacity"], splats["scaling"], parent, MIN_OPACITY).any()
        mcmc.move_rows(splats["means"], parent, dead_idx, 300)
        assert all(torch.equal(splats[k], before[k]) for k in splats)


# ---- move and zero_rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("w", [1, 3, 48, 1025])
def test_move_and_zero_rows(dev, w, strided):
    n, m = 1500, 1100  # more rows than one workgroup takes at every width
    r = np.random.default_rng(w)
    perm = r.permutation(n)
    dead_idx = np.sort(perm[:m]).astype(np.int32)
    parent = np.sort(r.choice(perm[m:], size=m)).astype(np.int32)
    table = ref.f32(r.normal(size=(n, w + (7 if strided else 0))))
    dev_table = up(table, dev)
    view = dev_table[:, :w]
    mcmc.move_rows(view, up(parent, dev), up(dead_idx, dev), n)
    want = table.copy()
    want[:, :w] = ref.move(table[:, :w], parent, dead_idx)
    assert same_bits(dev_table.cpu().numpy(), want)  # (the columns beyond w are untouched)
    count = np.zeros(n, np.int32)
    count[parent] = 1
    count[::7] = 0
    mcmc.zero_rows(view, up(count, dev))
    want[:, :w] = ref.zero_rows(want[:, :w], count)
    assert same_bits(dev_table.cpu().numpy(), want) and (count > 0).sum() > 50
    # a table with more rows than count: the rows beyond it stay
    tall = up(table, dev)
    mcmc.zero_rows(tall[:, :w], up(np.ones(100, np.int32), dev))
    assert not tall[:100, :w].any() and same_bits(tall[100:].cpu().numpy(), table[100:])


# ---- the rounds through the public interface --------------------------------------------------------------------------------------
def adam_setup(dev, t, keys=("means", "scaling", "opacity")):
    params = {k: up(v, dev).requires_grad_(True) for k, v in t.items() if k != "field"}
    opt = torch.optim.Adam([dict(params=[params[k]], lr=1e-3) for k in keys], eps=1e-15)
    loss = sum((params[k] ** 2).sum() for k in keys)
    loss.backward()
    opt.step()
    opt.zero_grad(set_to_none=True)
    return params, opt


def finite_scene(n=2000):
    t = scene(n)
    t["opacity"] = np.nan_to_num(t["opacity"], nan=-9.0)
    return t


def test_relocate_with_an_optimiser(dev):
    lib = DeviceLib(dev)
    t = finite_scene()
    n = len(t["opacity"])
    cfg = gsbp_amd.MCMCConfig()
    results = []
    for _ in range(2):  # twice from the same state and seed: the same bits
        params, opt = adam_setup(dev, t)
        ids = {k: id(v) for k, v in params.items()}
        t_now = {k: v.detach().cpu().numpy().copy() for k, v in params.items()}
        mom = {k: {m: opt.state[params[k]][m].clone() for m in ("exp_avg", "exp_avg_sq")} for k in ("means", "scaling", "opacity")}
        field = up(t["field"], dev)
        out, info = gsbp_amd.relocate(params, cfg, optimizer=opt, carry=dict(field=field), generator=torch.Generator(device=dev).manual_seed(77))
        results.append((out, info, opt, mom, t_now, field, ids))
    out, info, opt, mom, t_now, field, ids = results[0]
    assert out is not None and all(id(out[k]) == ids[k] for k in ids) and all(out[k].is_leaf and out[k].requires_grad for k in ids)
    parent, dead_idx, count = info["parent"].cpu().numpy(), info["dead_idx"].cpu().numpy(), info["count"].cpu().numpy()
    want_cdf, want_off, want_idx = ref.plan(t_now["opacity"], T_OPA, lib=lib)
    assert info["relocated"] == info["n_dead"] == len(want_idx) > 100 and info["total_weight"] == int(want_cdf[-1])
    assert np.array_equal(dead_idx, want_idx) and (np.diff(parent) >= 0).all() and np.array_equal(count, ref.counts(parent, n))
    assert count[dead_idx].sum() == 0
    want_o, want_s, _ = ref.update(t_now["opacity"], t_now["scaling"], parent, MIN_OPACITY, lib)
    want = dict(t_now, opacity=want_o, scaling=want_s, field=t["field"])
    got = dict({k: v.detach() for k, v in out.items()}, field=info["carry"]["field"])
    for k in want:
        assert same_bits(got[k].cpu().numpy(), ref.move(want[k], parent, dead_idx)), k
    assert info["carry"]["field"] is field
    for k, ms in mom.items():
        for name, old in ms.items():
            now = opt.state[out[k]][name]
            assert not now[count > 0].any() and torch.equal(now[count == 0], old[count == 0]), (k, name)  # parents zero, ...
            assert torch.equal(now[dead_idx], old[dead_idx]) and bool(old[dead_idx].any())                # ... dead rows untouched
    again = results[1]
    assert all(torch.equal(again[0][k], out[k]) for k in ids) and torch.equal(again[1]["parent"], info["parent"])
    sum((out[k] ** 2).sum() for k in ids).backward()
    opt.step()  # the optimiser still runs on the same parameter objects
    assert float(opt.state[out["means"]]["step"]) == 2.0


def test_sample_add_with_an_optimiser(dev):
    lib = DeviceLib(dev)
    t = finite_scene()
    n = len(t["opacity"])
    cfg = gsbp_amd.MCMCConfig(cap_max=2080)
    k_new = cfg.n_new(n)
    assert k_new == 80
    results = []
    for _ in range(2):
        params, opt = adam_setup(dev, t)
        t_now = {k: v.detach().cpu().numpy().copy() for k, v in params.items()}
        mom = {k: opt.state[params[k]]["exp_avg"].clone() for k in ("means", "scaling", "opacity")}
        out, info = gsbp_amd.sample_add(params, cfg, k_new, optimizer=opt, carry=dict(field=up(t["field"], dev)),
                                        generator=torch.Generator(device=dev).manual_seed(5))
        results.append((out, info, opt, mom, t_now, params))
    out, info, opt, mom, t_now, old = results[0]
    parent, count = info["parent"].cpu().numpy(), info["count"].cpu().numpy()
    assert (info["added"], info["n_before"], info["n_after"]) == (k_new, n, n + k_new) and len(parent) == k_new
    assert (np.diff(parent) >= 0).all() and np.array_equal(count, ref.counts(parent, n))
    want_o, want_s, _ = ref.update(t_now["opacity"], t_now["scaling"], parent, MIN_OPACITY, lib)
    want = dict(t_now, opacity=want_o, scaling=want_s, field=t["field"])
    got = dict({k: v.detach() for k, v in out.items()}, field=info["carry"]["field"])
    for k in want:
        assert same_bits(got[k].cpu().numpy(), np.concatenate([want[k], want[k][parent]])), k
    for k in ("means", "scaling", "opacity"):  # the leaves are swapped, the old ones untouched
        assert out[k] is not old[k] and out[k].is_leaf and out[k].requires_grad and opt.param_groups[["means", "scaling", "opacity"].index(k)]["params"][0] is out[k]
        assert same_bits(old[k].detach().cpu().numpy(), t_now[k]) and old[k] not in opt.state
        st = opt.state[out[k]]
        assert float(st["step"]) == 1.0 and tuple(st["exp_avg"].shape) == tuple(out[k].shape) == tuple(st["exp_avg_sq"].shape)
        assert not st["exp_avg"][n:].any() and not st["exp_avg_sq"][n:].any()                 # appended rows: zero
        assert not st["exp_avg"][:n][count > 0].any() and not st["exp_avg_sq"][:n][count > 0].any()  # parents: zero
        assert torch.equal(st["exp_avg"][:n][count == 0], mom[k][count == 0]) and bool(mom[k][count > 0].any())
    again = results[1]
    assert all(torch.equal(again[0][k], v) for k, v in out.items()) and torch.equal(again[1]["parent"], info["parent"])
    sum((out[k] ** 2).sum() for k in ("means", "scaling", "opacity")).backward()
    opt.step()
    same, none = gsbp_amd.sample_add(out, cfg, 0, optimizer=opt)
    assert same is out and none["added"] == 0


# ---- the statistics ------------------------------------------------------------------------------------------------------------------
def test_sampling_follows_the_weights(dev):
    opacity, u = sampling_case()
    cdf, _, _ = mcmc.plan(up(opacity, dev), -10.0, "relocate")
    parent = mcmc.draw(cdf, up(u, dev))
    count = mcmc.update(up(opacity, dev), torch.zeros(4, 3, device=dev), parent, MIN_OPACITY).cpu().numpy()
    check_sampling(count)
    assert np.array_equal(parent.cpu().numpy(), ref.draw(cdf.cpu().numpy(), u))


def test_noise_bit_for_bit_and_its_gate(dev):
    lib = DeviceLib(dev)
    means, scaling, rotation, opacity, z = noise_rows()
    scaler = 1.6e-4 * 5e5
    moved = up(means, dev)
    mcmc.add_noise(moved, up(scaling, dev), up(rotation, dev), up(opacity, dev), up(z, dev), scaler)
    got = moved.cpu().numpy()
    assert same_bits(got, ref.noise(means, scaling, rotation, opacity, z, scaler, lib))
    assert np.array_equal(got[0], means[0])  # logit 10: it moves by less than 1e-30 of its scale -- here, not at all
    assert np.abs(got[0].astype(np.float64) - means[0]).max() < 1e-30 * np.exp(scaling[0]).max()
    bound = ref.noise_bound(means, scaling, opacity, z, scaler)
    ratio = np.abs(got.astype(np.float64) - ref.literal_inject_noise(means, scaling, rotation, opacity, z, scaler)) / bound
    print(f"device noise against the float64 covariance form: largest error / bound = {ratio.max():.3f}")
    assert ratio.max() < 1.0


def test_noise_variance_of_a_transparent_gaussian(dev):
    means, scaling, rotation, opacity, z, scaler, want_var = noise_variance_case()
    moved = up(means, dev)
    mcmc.add_noise(moved, up(scaling, dev), up(rotation, dev), up(opacity, dev), up(z, dev), scaler)
    check_noise_variance(moved.cpu().numpy(), want_var)


def test_inject_noise_is_seeded(dev):
    t = finite_scene(500)
    cfg = gsbp_amd.MCMCConfig()
    outs = []
    for _ in range(2):
        splats = {k: up(v, dev) for k, v in t.items() if k != "field"}
        gsbp_amd.inject_noise(splats, 1.6e-4, cfg, generator=torch.Generator(device=dev).manual_seed(9))
        outs.append(splats["means"])
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], up(t["means"], dev))
    z = torch.randn(500, 3, generator=torch.Generator(device=dev).manual_seed(9), device=dev).cpu().numpy()
    want = ref.noise(t["means"], t["scaling"], t["rotation"], t["opacity"], z, 1.6e-4 * 5e5, DeviceLib(dev))
    assert same_bits(outs[0].cpu().numpy(), want)


# ---- training ----------------------------------------------------------------------------------------------------------------------------
def test_train_scene_under_the_strategy(dev):
    cfg, start, K, vms, images = t0_training_setup(dev)
    n0 = start["means"].shape[0]
    cap = 290
    strategy = gsbp_amd.MCMCConfig(refine_start_iter=5, refine_every=10, cap_max=cap)

    def run(**kw):
        return gsbp_amd.train_scene(start, vms, K, cfg.width, cfg.height, lambda v: images[v], 40, seed=3, **kw)
    trained, hist = run(strategy=strategy, opacity_reg=0.01, scale_reg=0.01)
    sizes, rounds = hist["n"], hist["rounds"]
    assert [r["step"] for r in rounds] == [10, 20, 30] and hist["resets"] == []
    assert sizes[0] == n0 and max(sizes) <= cap and trained["means"].shape[0] == cap == rounds[-1]["n_after"]
    for r in rounds:
        assert r["added"] == r["n_after"] - r["n_before"] == min(cap, int(1.05 * r["n_before"])) - r["n_before"]
        assert sizes[r["step"] + 1] == r["n_after"] and r["relocated"] >= 0
    assert rounds[0]["added"] == int(1.05 * n0) - n0 > 0 and rounds[-1]["added"] < int(1.05 * rounds[-1]["n_before"]) - rounds[-1]["n_before"]
    assert all(math.isfinite(v) for v in hist["loss"]) and hist["loss"][-1] < hist["loss"][0]
    assert all(bool(torch.isfinite(trained[k]).all()) for k in ("means", "scaling", "rotation", "opacity", "features_dc"))
    print(f"T0 under MCMC, 40 steps: N {n0} -> {trained['means'].shape[0]}, loss {hist['loss'][0]:.4f} -> {hist['loss'][-1]:.4f}, "
          f"relocated {[r['relocated'] for r in rounds]}")


def test_the_default_path_is_unchanged(dev):
    """strategy=None gives the loss history of the call without the keyword, bit for bit: T0's Gaussians and cameras, 40 steps, all six
    parameters, the same seed -- on the 32 x 16 pixels at the centre of T0's views.
    Why not the whole 96 x 64 view: there two IDENTICAL calls without the keyword do not give the same bits.  The blend backward adds a
    Gaussian's gradient over the tiles it touches with float atomics, in an order that differs from run to run
    (tests/test_gpu_blend_grad.py); measured on an MI355X, two such calls part at step 8 of 40 with all six parameters, and with the
    opacities and colours alone they agreed in one session and parted at step 28 in the next.  No comparison of loss bits can hold
    there, whatever this keyword does.  On two tiles it can: a Gaussian's gradient is then the sum of at most two partial sums onto
    zero, and a + b = b + a in floating point, so the training is reproducible by construction and every bit of the history counts."""
    cfg, start, K, vms, images = t0_training_setup(dev)
    w, h = 32, 16
    x0, y0 = (cfg.width - w) // 2, (cfg.height - h) // 2
    Kc = K.clone()
    Kc[0, 2] -= x0
    Kc[1, 2] -= y0
    crops = [im[y0:y0 + h, x0:x0 + w].contiguous() for im in images]

    def run(**kw):
        return gsbp_amd.train_scene(start, vms, Kc, w, h, lambda v: crops[v], 40, seed=3, **kw)[1]
    plain, none = run(), run(strategy=None)
    assert len(plain["loss"]) == 40 and plain["loss"] == none["loss"] and plain["n"] == none["n"] and plain["rounds"] == none["rounds"]
    assert plain["loss"][-1] < plain["loss"][0] and len(set(plain["loss"])) == 40  # it trains: the bits compared are not a constant's
    dcfg = gsbp_amd.DensifyConfig(refine_start_iter=5, refine_every=10)  # ... and with rounds on the way, under either keyword
    a, b = run(cfg=dcfg), run(strategy=dcfg)
    assert a["loss"] == b["loss"] and a["n"] == b["n"] and [r["step"] for r in a["rounds"]] == [10, 20, 30] and a["rounds"] == b["rounds"]


# ---- what the host cannot check ------------------------------------------------------------------------------------------------------
def test_garbage_in_range_writes_nothing_out_of_range(dev):
    """An unsorted u gives an unsorted parent: the counts are then wrong, and every write still lands in its own row; parents and dead
    rows outside [0, n) move nothing.  Guard rows around every table show it."""
    n, m, pad = 700, 900, 64
    r = np.random.default_rng(1)
    t = finite_scene(n)
    cdf, _, _ = mcmc.plan(up(t["opacity"], dev), T_OPA, "relocate")
    parent = mcmc.draw(cdf, up(r.random(m), dev))  # not sorted
    assert bool((parent >= 0).all()) and bool((parent < n).all()) and not bool((parent[1:] >= parent[:-1]).all())
    guard_o = torch.full((n + 2 * pad,), 7.0, device=dev)
    guard_s = torch.full((n + 2 * pad, 3), 7.0, device=dev)
    guard_o[pad:pad + n], guard_s[pad:pad + n] = up(t["opacity"], dev), up(t["scaling"], dev)
    count = mcmc.update(guard_o[pad:pad + n], guard_s[pad:pad + n], parent, MIN_OPACITY)
    assert bool((count >= 0).all()) and int(count.sum()) <= m
    for g in (guard_o, guard_s):
        assert bool((g[:pad] == 7.0).all()) and bool((g[pad + n:] == 7.0).all())
    table = torch.full((n + 2 * pad, 5), 7.0, device=dev)
    table[pad:pad + n] = up(t["field"], dev)
    wild = up(r.integers(-5, n + 5, size=m).astype(np.int32), dev)  # in-range values with a few beyond either end
    mcmc.move_rows(table[pad:pad + n], wild, up(r.integers(-5, n + 5, size=m).astype(np.int32), dev), n)
    mcmc.move_rows(table[pad:pad + n], parent, wild, n)
    assert bool((table[:pad] == 7.0).all()) and bool((table[pad + n:] == 7.0).all())
    # the C ABI's refusals with device arrays in hand: nothing is launched
    lib = _lib.lib()
    good = torch.zeros(64, device=dev)
    assert lib.gwbp_mcmc_draw(4, -1, ptr(cdf), ptr(good), ptr(good), None) == -1
    assert lib.gwbp_mcmc_draw(4, 4, ptr(cdf), C.c_void_p(good.data_ptr() + 4), ptr(good), None) == -1
    assert lib.gwbp_mcmc_move(4, 4, 3, ptr(good), ptr(good), ptr(good), 2, None) == -1
    assert lib.gwbp_mcmc_move(4, 4, 3, None, ptr(good), ptr(good), 3, None) == -1
    assert lib.gwbp_mcmc_zero_rows(4, 3, ptr(good), C.c_void_p(good.data_ptr() + 2), 3, None) == -1
    torch.cuda.synchronize(dev)
