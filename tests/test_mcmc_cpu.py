"""No-GPU checks of the MCMC strategy: csrc/mcmc_math.h compiled for the host -- plainly and under
-fsanitize=address,undefined, a stand-alone program both times -- against the numpy yardstick bit for bit; the yardstick's fused form
against gsplat's literal rule in float64 (identical rows, parents and counts; o', s' and the noise inside bounds DERIVED in
mcmc_ref.py, the measured fraction printed); the mutants the comparison must catch; the sampling and noise statistics of the seeds the
GPU tests use; the configuration, the C ABI's argument checks and what the Python layer refuses without a device.
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

import mcmc_ref as ref
import gsbp_amd
from gsbp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_OPACITY = 0.005
SAMPLING_SEED, NOISE_SEED = 7, 11  # the seeds tests/test_gpu_mcmc.py uses as well: verified here against the reference


# ---- the data ----------------------------------------------------------------------------------------------------------------------
def scene(n=2000, seed=5, dead=0.15, extra=5):
    """Pre-activation tables with about `dead` of the opacities at or below logit(min_opacity), one NaN among them."""
    r = np.random.default_rng(seed)
    t = dict(means=ref.f32(r.normal(size=(n, 3))), scaling=ref.f32(math.log(0.05) + 0.7 * r.normal(size=(n, 3))),
             rotation=ref.f32(r.normal(size=(n, 4))), opacity=ref.f32(1.5 * r.normal(size=n) - 1.0), field=ref.f32(r.normal(size=(n, extra))))
    gone = r.random(n) < dead
    t["opacity"][gone] = ref.f32(-5.3 - 3.0 * r.random(int(gone.sum())))
    t["opacity"][0], t["opacity"][n - 1] = -9.0, -7.0        # the first and the last row are dead
    t["opacity"][3] = np.float32(ref.logit(float(np.float32(MIN_OPACITY))))  # exactly the threshold: dead (<=)
    t["opacity"][n // 2] = np.nan
    return t


def heavy_scene(n=300, n_dead=200):
    """One almost opaque Gaussian among barely alive ones: it takes most of the draws, so that its ratio clamps at 51."""
    t = scene(n, seed=8, dead=0.0)
    t["opacity"][:] = -5.0
    t["opacity"][:n_dead] = -8.0
    t["opacity"][n - 7] = 8.0
    return t


def moments_of(t, seed=9):
    r = np.random.default_rng(seed)
    return {k: ref.f32(r.normal(size=np.asarray(t[k]).shape)) + np.float32(10.0) for k in ("means", "opacity", "scaling")}  # never zero


def sorted_u(m, seed):
    return np.sort(np.random.default_rng(seed).random(m))


def check_round_against_literal(fused, literal, parents, t0, min_opacity=MIN_OPACITY):
    """The geometry of the parents inside the derived bounds, everything else identical; returns the largest error / bound."""
    worst = 0.0
    hit = np.unique(parents)
    c = np.bincount(parents, minlength=len(t0["opacity"]))[hit]
    b_logit, b_s = ref.relocation_bounds(t0["opacity"][hit], t0["scaling"][hit], np.minimum(c + 1, ref.MAX_RATIO), min_opacity)
    worst = max(worst, float((np.abs(fused["opacity"][hit].astype(np.float64) - literal["opacity"][hit]) / b_logit).max()))
    worst = max(worst, float((np.abs(fused["scaling"][hit].astype(np.float64) - literal["scaling"][hit]) / b_s).max()))
    return worst


# ---- the fused form against the literal rule -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["plain", "heavy"])
def test_the_fused_relocate_round_yields_the_rows_of_the_literal_rule(which):
    t = scene() if which == "plain" else heavy_scene()
    n = len(t["opacity"])
    mom = moments_of(t)
    u = sorted_u(n, 3)
    new, new_mom, parent, dead_idx, count = ref.relocate_round(t, mom, MIN_OPACITY, u)
    m = len(dead_idx)
    assert m > 10 and len(parent) == m and (np.diff(parent) >= 0).all()
    # the draws are the rule's: an inverse CDF over the exact float64 probabilities of the ALIVE Gaussians gives the same parents
    assert np.array_equal(parent, ref.literal_parents(t["opacity"], MIN_OPACITY, u[:m]))
    assert not np.isin(parent, dead_idx).any()
    lit, lit_mom, lit_dead, lit_count = ref.literal_relocate(t, mom, MIN_OPACITY, parent)
    assert np.array_equal(dead_idx, lit_dead) and np.array_equal(count, lit_count)
    if which == "heavy":
        assert count.max() >= 60  # the ratio clamps at 51
    else:
        assert {0, 3, n // 2, n - 1} <= set(dead_idx)  # the first and the last row, the threshold itself and the NaN are dead
    # rows: untouched rows keep their bits, dead rows are their parents' rows, moments as the rule says
    changed = np.zeros(n, bool)
    changed[dead_idx], changed[parent] = True, True
    for k in t:
        assert np.array_equal(new[k][~changed].view(np.uint32), t[k][~changed].view(np.uint32)), k
        assert np.array_equal(new[k][dead_idx].view(np.uint32), new[k][parent].view(np.uint32)), k
        assert np.array_equal(lit[k][dead_idx], lit[k][parent]), k
        if k not in ("opacity", "scaling"):
            assert np.array_equal(new[k].astype(np.float64), lit[k], equal_nan=True), k
    for k in mom:
        assert np.array_equal(new_mom[k], lit_mom[k]), k
        assert not new_mom[k][parent].any() and np.array_equal(new_mom[k][dead_idx], mom[k][dead_idx])
    worst = check_round_against_literal(new, lit, parent, t)
    print(f"relocate ({which}): o' and s' of {len(np.unique(parent))} parents, float32 fused against float64 literal: largest error / "
          f"bound = {worst:.3f}")
    assert worst < 1.0


def test_the_fused_add_round_yields_the_rows_of_the_literal_rule():
    t = scene()
    n = len(t["opacity"])
    mom = moments_of(t)
    k_new = ref.n_new(n, 10 ** 6)
    assert k_new == int(1.05 * n) - n == 100
    u = sorted_u(k_new, 4)
    new, new_mom, parent, count = ref.add_round(t, mom, MIN_OPACITY, u)
    assert np.array_equal(parent, ref.literal_parents(t["opacity"], MIN_OPACITY, u, alive_only=False))
    lit, lit_mom, lit_count = ref.literal_sample_add(t, mom, MIN_OPACITY, parent)
    assert np.array_equal(count, lit_count) and all(len(v) == n + k_new for v in new.values())
    for k in t:
        assert np.array_equal(new[k][n:].view(np.uint32), new[k][parent].view(np.uint32)), k
        if k not in ("opacity", "scaling"):
            assert np.array_equal(new[k].astype(np.float64), lit[k], equal_nan=True), k
    for k in mom:
        assert np.array_equal(new_mom[k], lit_mom[k]) and not new_mom[k][n:].any() and not new_mom[k][parent].any()
    worst = check_round_against_literal(new, lit, parent, t)
    print(f"sample_add: largest error / bound = {worst:.3f}")
    assert worst < 1.0
    assert ref.n_new(1000, 1020) == 20 and ref.n_new(1000, 900) == 0 and ref.n_new(19, 100) == 0


def test_relocation_at_every_ratio_against_the_literal_formula():
    """o' and s' at ratios 1 .. 51 and opacities from barely alive to almost opaque."""
    r = np.random.default_rng(12)
    ratio = np.tile(np.arange(1, ref.MAX_RATIO + 1), 8)
    m = len(ratio)
    opacity = ref.f32(np.concatenate([r.uniform(-5.2, 3.0, m - 2 * ref.MAX_RATIO), r.uniform(3.0, 9.0, 2 * ref.MAX_RATIO)]))
    scaling = ref.f32(math.log(0.05) + r.normal(size=(m, 3)))
    o32, s32 = ref.relocate_values(opacity, scaling, ratio, MIN_OPACITY)
    o = 1.0 / (1.0 + np.exp(-opacity.astype(np.float64)))
    on, sn = ref.literal_compute_relocation(o, np.exp(scaling.astype(np.float64)), ratio)
    on = np.clip(on, float(np.float32(MIN_OPACITY)), 1.0 - 2.0 ** -23)
    b_logit, b_s = ref.relocation_bounds(opacity, scaling, ratio, MIN_OPACITY)
    e_o = np.abs(o32.astype(np.float64) - np.log(on / (1.0 - on))) / b_logit
    e_s = np.abs(s32.astype(np.float64) - np.log(sn)) / b_s
    print(f"ratios 1..51: largest error / bound: opacity {e_o.max():.3f}, scale {e_s.max():.3f} (at ratio {ratio[e_s.max(axis=1).argmax()]})")
    assert e_o.max() < 1.0 and e_s.max() < 1.0
    # ratio 1 changes nothing but roundings: o' = o, D = o', s' = s
    one = ratio == 1
    assert np.abs(s32[one] - scaling[one]).max() < 1e-5 and np.abs(o32[one] - opacity[one]).max() < 1e-3


def noise_rows(n=4000, seed=13):
    r = np.random.default_rng(seed)
    means = ref.f32(r.normal(size=(n, 3)) * 3.0)
    scaling = ref.f32(math.log(0.05) + r.normal(size=(n, 3)))
    rotation = ref.f32(r.normal(size=(n, 4)))
    opacity = ref.f32(r.uniform(-9.0, -3.0, size=n))  # 1 - o from 0.95 to 0.9999: the gate's whole rise
    opacity[:5] = [10.0, 3.0, 0.0, -20.0, -5.3]
    z = ref.f32(r.normal(size=(n, 3)))
    return means, scaling, rotation, opacity, z


def test_noise_against_the_literal_covariance_form():
    means, scaling, rotation, opacity, z = noise_rows()
    scaler = 1.6e-4 * 5e5
    got = ref.noise(means, scaling, rotation, opacity, z, scaler)
    want = ref.literal_inject_noise(means, scaling, rotation, opacity, z, scaler)
    ratio = np.abs(got.astype(np.float64) - want) / ref.noise_bound(means, scaling, opacity, z, scaler)
    print(f"noise, float32 fused against float64 M M^T: largest error / bound = {ratio.max():.3f}, median {np.median(ratio):.4f}")
    assert got.dtype == np.float32 and ratio.max() < 1.0
    moved = np.abs(want - means).max(axis=1)
    assert moved[0] == 0.0 or moved[0] < 1e-30 * np.exp(scaling[0].astype(np.float64)).max()  # opaque: the gate is shut
    assert np.array_equal(got[0], means[0])
    assert np.median(moved[5:]) > 1e-4  # transparent ones do move


# ---- mutants ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", ["ratio_no_plus_one", "clamp_50", "dead_keep_weight", "zero_dead_moments", "gate_o"])
def test_mutants_fail(mutant):
    if mutant == "gate_o":
        means, scaling, rotation, opacity, z = noise_rows()
        got = ref.noise(means, scaling, rotation, opacity, z, 80.0, mutant=mutant)
        want = ref.literal_inject_noise(means, scaling, rotation, opacity, z, 80.0)
        ratio = np.abs(got.astype(np.float64) - want) / ref.noise_bound(means, scaling, opacity, z, 80.0)
        assert np.median(ratio) > 100.0
        return
    t = heavy_scene()
    mom = moments_of(t)
    u = sorted_u(len(t["opacity"]), 3)
    new, new_mom, parent, dead_idx, count = ref.relocate_round(t, mom, MIN_OPACITY, u, mutant=mutant)
    if mutant == "dead_keep_weight":
        assert not np.array_equal(parent, ref.literal_parents(t["opacity"], MIN_OPACITY, u[:len(dead_idx)]))
        assert np.isin(parent, dead_idx).any()
        return
    lit, lit_mom, _, _ = ref.literal_relocate(t, mom, MIN_OPACITY, parent)
    if mutant == "zero_dead_moments":
        assert not all(np.array_equal(new_mom[k], lit_mom[k]) for k in mom)
        return
    assert count.max() >= 60
    assert check_round_against_literal(new, lit, parent, t) > 10.0


# ---- the statistics of the seeds the GPU tests use --------------------------------------------------------------------------------------
def sampling_case():
    opacity = ref.f32([ref.logit(p) for p in (0.1, 0.2, 0.3, 0.4)])
    return opacity, sorted_u(40_000, SAMPLING_SEED)


def check_sampling(count):
    m, p = 40_000, np.array([0.1, 0.2, 0.3, 0.4])
    assert count.sum() == m
    dev = np.abs(count - m * p) / np.sqrt(m * p * (1.0 - p))
    assert dev.max() < 5.0, dev
    return dev


def test_sampling_follows_the_weights():
    opacity, u = sampling_case()
    cdf, _, _ = ref.plan(opacity, -10.0)
    w = np.diff(cdf)
    assert np.abs(w / w.sum() - [0.1, 0.2, 0.3, 0.4]).max() < 1e-6  # the quantisation: 2^-24 / p
    dev = check_sampling(ref.counts(ref.draw(cdf, u), 4))
    print(f"sampling, seed {SAMPLING_SEED}: deviations in sigma {np.round(dev, 2)}")
    # the edges of a draw: u = 0 the first alive Gaussian, u -> 1 the last; a zero-weight Gaussian is never drawn
    cdf = np.array([0, 0, 5, 5, 9, 9], np.int64)
    assert ref.draw(cdf, np.array([0.0, 0.5, 0.5555, 0.5556, 0.999999, 1.0, 7.0, -1.0, np.nan])).tolist() == [1, 1, 1, 3, 3, 3, 3, 1, 1]
    assert ref.draw(np.zeros(4, np.int64), np.array([0.3])).tolist() == [-1]


def noise_variance_case(n=40_000):
    """n copies of one transparent Gaussian, long along x: (means, scaling, rotation, opacity, z, scaler, the expected variance)."""
    z = ref.f32(np.random.default_rng(NOISE_SEED).normal(size=(n, 3)))
    scaling = np.tile(ref.f32([math.log(1.0), math.log(0.1), math.log(0.1)]), (n, 1))
    rotation = np.tile(ref.f32([1.0, 0.0, 0.0, 0.0]), (n, 1))
    opacity = np.full(n, -10.0, np.float32)
    o = 1.0 / (1.0 + math.exp(10.0))
    g = 1.0 / (1.0 + math.exp(-100.0 * ((1.0 - o) - 0.995)))
    scaler = 0.05
    return np.zeros((n, 3), np.float32), scaling, rotation, opacity, z, scaler, (g * scaler) ** 2 * np.array([1.0, 1e-4, 1e-4])


def check_noise_variance(moved, want_var):
    n = len(moved)
    var = (moved.astype(np.float64) ** 2).mean(axis=0)
    dev = np.abs(var - want_var) / (want_var * math.sqrt(2.0 / n))
    assert dev.max() < 5.0, dev
    assert var[0] > 5000.0 * var[1]  # along the longest axis
    return dev


def test_noise_variance_of_a_transparent_gaussian():
    means, scaling, rotation, opacity, z, scaler, want_var = noise_variance_case()
    dev = check_noise_variance(ref.noise(means, scaling, rotation, opacity, z, scaler), want_var)
    print(f"noise variance, seed {NOISE_SEED}: deviations in sigma {np.round(dev, 2)}")


# ---- the header on the host ------------------------------------------------------------------------------------------------------------
class HostLib:
    """expf, logf and powf of the host's libm, through tests/mcmc_host.cpp."""

    def __init__(self, exe, tmp):
        self.exe, self.tmp, self.calls = exe, str(tmp), 0

    def _run(self, op, a, b=None):
        a = ref.f32(a)
        b = np.zeros_like(a) if b is None else ref.f32(np.broadcast_to(b, a.shape))
        self.calls += 1
        src, dst = os.path.join(self.tmp, "libm_in.bin"), os.path.join(self.tmp, "libm_out.bin")
        with open(src, "wb") as f:
            f.write(struct.pack("<qi", a.size, op) + a.tobytes() + b.tobytes())
        subprocess.check_call([self.exe, "libm", src, dst])
        return np.fromfile(dst, np.float32).reshape(a.shape)

    def exp(self, a):
        return self._run(0, a)

    def log(self, a):
        return self._run(1, a)

    def pow(self, a, b):
        return self._run(2, a, b)


@pytest.fixture(scope="module")
def host_programs(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (c++, g++, clang++) found")
    d = tmp_path_factory.mktemp("mcmc_host")
    base = [cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"]
    src = os.path.join(ROOT, "tests", "mcmc_host.cpp")
    plain, checked = str(d / "mcmc_host"), str(d / "mcmc_host_san")
    subprocess.check_call(base + ["-O2", "-o", plain, src])
    subprocess.check_call(base + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", checked, src])
    return plain, checked, d


def host_rows(n=4001, seed=21):
    t = scene(n, seed)
    r = np.random.default_rng(seed + 1)
    ratio = r.integers(1, ref.MAX_RATIO + 1, size=n).astype(np.int32)
    ratio[:ref.MAX_RATIO] = np.arange(1, ref.MAX_RATIO + 1)
    t["opacity"][10:16] = [20.0, -20.0, 9.0, np.inf, -np.inf, 0.0]
    z = ref.f32(r.normal(size=(n, 3)))
    return t, ratio, z


def run_math(exe, tmp, t, ratio, z, scaler, t_opa):
    n = len(ratio)
    src, dst = os.path.join(str(tmp), "math_in.bin"), os.path.join(str(tmp), "math_out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<q3f", n, MIN_OPACITY, t_opa, scaler))
        f.write(t["opacity"].tobytes() + t["scaling"].tobytes() + ratio.tobytes() + t["means"].tobytes() + t["rotation"].tobytes() + z.tobytes())
    subprocess.check_call([exe, "math", src, dst])
    raw = open(dst, "rb").read()
    assert len(raw) == n * (8 + 4 * (1 + 3 + 1 + 3))
    return dict(weight=np.frombuffer(raw, np.int64, n), opacity=np.frombuffer(raw, np.float32, n, 8 * n),
                scaling=np.frombuffer(raw, np.float32, 3 * n, 12 * n).reshape(n, 3), gate=np.frombuffer(raw, np.float32, n, 24 * n),
                moved=np.frombuffer(raw, np.float32, 3 * n, 28 * n).reshape(n, 3)), raw


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_mcmc_math_on_the_host(host_programs):
    plain, checked, tmp = host_programs
    t, ratio, z = host_rows()
    t_opa, scaler = float(np.float32(ref.logit(float(np.float32(MIN_OPACITY))))), 80.0
    got, raw = run_math(plain, tmp, t, ratio, z, scaler, t_opa)
    lib = HostLib(plain, tmp)
    # with this libm's exp, log and pow the header is the restatement, bit for bit
    assert np.array_equal(got["weight"], ref.weights(t["opacity"], t_opa, lib))
    assert got["weight"][t["opacity"].shape[0] // 2] == 0 and got["weight"][13] == 1 << 24 and (got["weight"] > 0).sum() > 3000
    want_o, want_s = ref.relocate_values(t["opacity"], t["scaling"], ratio, MIN_OPACITY, lib)
    fin = np.isfinite(t["opacity"])
    assert same_bits(got["opacity"][fin], want_o[fin]) and same_bits(got["scaling"][fin], want_s[fin])
    assert same_bits(got["gate"][fin], ref.gate(t["opacity"], lib)[fin])
    assert same_bits(got["moved"][fin], ref.noise(t["means"], t["scaling"], t["rotation"], t["opacity"], z, scaler, lib)[fin])
    assert lib.calls > 8
    # the same text under the address and undefined-behaviour sanitizers: a clean run and the same bytes
    _, raw_checked = run_math(checked, tmp, t, ratio, z, scaler, t_opa)
    assert raw_checked == raw


def test_the_library_calls_within_their_documented_error(host_programs):
    """expf, logf and powf of the host against float64 on the same arguments: one unit in the last place (glibc documents 1 ulp)."""
    plain, checked, tmp = host_programs
    r = np.random.default_rng(2)
    a = ref.f32(r.uniform(-20.0, 20.0, 20000))
    p = ref.f32(r.uniform(1e-6, 1.0, 20000))
    e = ref.f32(1.0 / r.integers(1, 52, 20000))
    for lib in (HostLib(plain, tmp), HostLib(checked, tmp)):
        for got, want in ((lib.exp(a), np.exp(a.astype(np.float64))), (lib.log(p), np.log(p.astype(np.float64))),
                          (lib.pow(p, e), np.power(p.astype(np.float64), e.astype(np.float64)))):
            ulp = np.abs(got.astype(np.float64) - want) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
            assert ulp.max() <= 1.0, ulp.max()


# ---- the configuration -----------------------------------------------------------------------------------------------------------------
def test_config_validation_and_schedule():
    cfg = gsbp_amd.MCMCConfig()
    assert (cfg.cap_max, cfg.noise_lr, cfg.refine_start_iter, cfg.refine_stop_iter, cfg.refine_every, cfg.min_opacity) == \
        (1_000_000, 5e5, 500, 25_000, 100, 0.005)
    for bad in (dict(cap_max=0), dict(noise_lr=-1.0), dict(noise_lr=float("nan")), dict(min_opacity=0.0), dict(min_opacity=1.0),
                dict(refine_every=0), dict(refine_start_iter=-1), dict(refine_stop_iter=-1)):
        with pytest.raises(gsbp_amd.GwbpError):
            gsbp_amd.MCMCConfig(**bad)
    cfg = gsbp_amd.MCMCConfig(refine_start_iter=10, refine_every=10, refine_stop_iter=50)
    assert [s for s in range(80) if cfg.refines_at(s)] == [20, 30, 40]
    assert [s for s in range(0, 26_000, 100) if gsbp_amd.MCMCConfig().refines_at(s)] == list(range(600, 25_000, 100))
    assert cfg.t_opa() == float(np.float32(ref.logit(float(np.float32(0.005)))))
    assert (cfg.n_new(2000), gsbp_amd.MCMCConfig(cap_max=2050).n_new(2000), gsbp_amd.MCMCConfig(cap_max=100).n_new(2000)) == (100, 50, 0)
    assert all(cfg.n_new(n) == ref.n_new(n, cfg.cap_max) for n in range(0, 3000, 7))


# ---- the C ABI: nothing here reaches a kernel --------------------------------------------------------------------------------------
NAMES = ("gwbp_mcmc_plan_workspace_size", "gwbp_mcmc_plan", "gwbp_mcmc_draw", "gwbp_mcmc_update", "gwbp_mcmc_move", "gwbp_mcmc_zero_rows",
         "gwbp_mcmc_noise", "gwbp_mcmc_libm")


def test_header_declares_the_entry_points_and_the_library_exports_them():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gwbp.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(rf"GWBP_API int {name}\s*\(", src), name
        assert name in _lib.ARGTYPES
    gsbp_amd.build()
    assert all(hasattr(_lib.lib(), n) for n in NAMES)
    for name in ("MCMCConfig", "relocate", "sample_add", "inject_noise", "train_scene"):
        assert callable(getattr(gsbp_amd, name)), name


def test_capi_rejects_without_a_launch():
    lib = _lib.lib()
    buf = (C.c_double * 64)()
    a = C.addressof(buf)

    def message():
        return lib.gwbp_last_error_string().decode()

    need = C.c_size_t(0)
    assert lib.gwbp_mcmc_plan_workspace_size(1000, C.byref(need)) == 0 and need.value == 2 * 8 * 4
    assert lib.gwbp_mcmc_plan_workspace_size(0, C.byref(need)) == 0 and need.value == 16
    assert lib.gwbp_mcmc_plan_workspace_size(65537, C.byref(need)) == 0 and need.value == 2 * 8 * 257
    assert lib.gwbp_mcmc_plan_workspace_size(-1, C.byref(need)) == -1 and lib.gwbp_mcmc_plan_workspace_size(4, None) == -1

    def plan(n=4, o=a, mode=0, cdf=a + 64, off=a + 128, idx=a + 192, ws=a + 256, ws_bytes=64):
        return lib.gwbp_mcmc_plan(n, o, -5.0, mode, cdf, off, idx, ws, ws_bytes, None)
    assert plan(n=-1) == -1 and "Gaussians" in message()
    assert plan(n=1 << 31) == -1
    assert plan(mode=2) == -1 and "mode" in message()
    for null in ("o", "cdf", "off", "idx", "ws"):
        assert plan(**{null: None}) == -1 and "null" in message(), null
    assert plan(cdf=a + 68) == -1 and "8-B" in message()
    assert plan(ws=a + 260) == -1 and plan(off=a + 132) == -1 and plan(o=a + 2) == -1 and plan(idx=a + 193) == -1
    assert plan(off=a + 64) == -1 and "same array" in message()
    assert plan(n=1000, ws_bytes=63) == -2 and "64" in message()

    def draw(n=4, m=4, cdf=a, u=a + 64, parent=a + 128):
        return lib.gwbp_mcmc_draw(n, m, cdf, u, parent, None)
    assert draw(n=-1) == -1 and draw(m=-1) == -1 and "draws" in message()
    assert draw(m=1 << 31) == -1
    for null in ("cdf", "u", "parent"):
        assert draw(**{null: None}) == -1 and "null" in message()
    assert draw(cdf=a + 4) == -1 and draw(u=a + 68) == -1 and "8-B" in message()
    assert draw(parent=a + 130) == -1 and "4-B" in message()
    assert draw(m=0, cdf=None, u=None, parent=None) == 0 and draw(n=0, m=3) == 0  # nothing to draw (from): no launch

    def update(n=4, m=4, parent=a, mo=0.005, o=a + 64, s=a + 128, lds=3, count=a + 256):
        return lib.gwbp_mcmc_update(n, m, parent, mo, o, s, lds, count, None)
    assert update(n=-1) == -1 and update(m=-1) == -1
    assert update(mo=0.0) == -1 and update(mo=1.0) == -1 and update(mo=float("nan")) == -1 and "min_opacity" in message()
    assert update(lds=2) == -1 and "stride" in message()
    for null in ("parent", "o", "s", "count"):
        assert update(**{null: None}) == -1 and "null" in message()
    assert update(o=a + 66) == -1 and update(parent=a + 1) == -1 and update(count=a + 258) == -1 and "aligned" in message()
    assert update(n=0, m=0, parent=None, o=None, s=None, count=None) == 0

    def move(n=4, m=4, w=3, parent=a, dead=a + 64, t=a + 128, ldt=3):
        return lib.gwbp_mcmc_move(n, m, w, parent, dead, t, ldt, None)
    assert move(n=-1) == -1 and move(m=-1) == -1
    for w in (0, -1, 65537):
        assert move(w=w) == -1 and "w must be" in message()
    assert move(ldt=2) == -1 and "stride" in message()
    for null in ("parent", "dead", "t"):
        assert move(**{null: None}) == -1 and "null" in message()
    assert move(t=a + 130) == -1 and move(parent=a + 2) == -1 and move(dead=a + 65) == -1 and "aligned" in message()
    assert move(m=0, parent=None, dead=None, t=None) == 0 and move(n=0, m=0) == 0

    def zero(n=4, w=3, count=a, t=a + 64, ldt=3):
        return lib.gwbp_mcmc_zero_rows(n, w, count, t, ldt, None)
    assert zero(n=-1) == -1 and zero(w=0) == -1 and zero(ldt=2) == -1
    assert zero(count=None) == -1 and zero(t=None) == -1 and "null" in message()
    assert zero(count=a + 2) == -1 and zero(t=a + 66) == -1 and "aligned" in message()
    assert zero(n=0, count=None, t=None) == 0

    def noise(n=4, m_=a, s=a + 64, q=a + 128, o=a + 192, z=a + 256):
        return lib.gwbp_mcmc_noise(n, m_, s, q, o, z, 1.0, None)
    assert noise(n=-1) == -1
    for null in ("m_", "s", "q", "o", "z"):
        assert noise(**{null: None}) == -1 and "null" in message()
    assert noise(m_=a + 2) == -1 and noise(z=a + 257) == -1 and "aligned" in message()
    assert noise(z=a) == -1 and "input" in message()
    assert noise(n=0, m_=None, s=None, q=None, o=None, z=None) == 0

    def libm(n=4, op=0, x=a, y=a + 64, out=a + 128):
        return lib.gwbp_mcmc_libm(n, op, x, y, out, None)
    assert libm(n=-1) == -1 and libm(op=3) == -1 and "op" in message()
    assert libm(x=None) == -1 and libm(out=None) == -1 and libm(op=2, y=None) == -1 and "null" in message()
    assert libm(x=a + 2) == -1 and libm(n=0) == 0
    del buf


# ---- the Python layer without a device ---------------------------------------------------------------------------------------------
def test_cpu_tensors_raise():
    sc = gsbp_amd.synthetic.make_scene(gsbp_amd.synthetic.CONFIGS["T0"])
    sc["features_dc"] = torch.zeros(512, 1, 3)
    cfg = gsbp_amd.MCMCConfig()
    for call in (lambda: gsbp_amd.relocate(sc, cfg), lambda: gsbp_amd.sample_add(sc, cfg, 10), lambda: gsbp_amd.inject_noise(sc, 1e-4, cfg),
                 lambda: gsbp_amd.train_scene(sc, torch.eye(4)[None], torch.eye(3), 96, 64, lambda v: None, 10, strategy=cfg)):
        with pytest.raises(gsbp_amd.GwbpError, match="no CPU path"):
            call()
    with pytest.raises(gsbp_amd.GwbpError, match="not both"):
        gsbp_amd.train_scene(sc, torch.eye(4)[None], torch.eye(3), 96, 64, lambda v: None, 10, gsbp_amd.DensifyConfig(), strategy=cfg)
    with pytest.raises(gsbp_amd.GwbpError, match="strategy must be"):
        gsbp_amd.train_scene(sc, torch.eye(4)[None], torch.eye(3), 96, 64, lambda v: None, 10, strategy="mcmc")
