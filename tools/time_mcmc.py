#!/usr/bin/env python3
"""The MCMC strategy at full size (C2 geometry: 1 000 000 Gaussians, 1600 x 1060, SH degree 3) in one run on one device, the forms of
each comparison alternating inside every repeat:

  noise_kernel     inject_noise: one torch.randn and gwbp_mcmc_noise
  noise_torch      the literal torch ops of the rule: sigmoid, exp, the rotation and covariance of every Gaussian, the gate, einsum
  round_kernels    relocate() + sample_add() with about 15 % of the Gaussians dead: six parameters and their Adam moments, the host read
                   included
  round_torch      gsplat's relocate and sample_add ported to device tensors: multinomial, bincount, the relocation formula from a
                   [51, 51] coefficient table, indexed assignment and cat over the same parameters and moments
  step_fixed       polish_scene's training step: render -> photometric_loss -> backward -> Adam step
  step_mcmc        the same step with the two regularisers in the loss and inject_noise behind it (what train_scene runs)
  step_noise_torch the same with noise_torch in place of the kernel

    timeout -k 10 900 python tools/time_mcmc.py --out profiles/mcmc.json

Each form is timed between one pair of hip events around work that ends in a synchronise; the record holds the median over --repeats
with min and max.  peak_mib is torch.cuda.max_memory_allocated over the form, above what was allocated before it.  Also recorded: PSNR
after equal steps of train_scene under the MCMC strategy, under the default strategy and of polish_scene on T1 from every second
Gaussian (recorded, not asserted).
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gsbp_amd  # noqa: E402,F401
import torch  # noqa: E402
from gsbp_amd import synthetic as syn  # noqa: E402
from gsbp_amd.polish import PARAM_KEYS, render_splats  # noqa: E402

from time_densify import KEYS, make_splats, optimizer_of, timed  # noqa: E402


def noise_torch(splats, lr, cfg, generator=None):
    """gsplat's inject_noise_to_position in torch ops."""
    with torch.no_grad():
        o = torch.sigmoid(splats["opacity"])
        scales = torch.exp(splats["scaling"])
        q = torch.nn.functional.normalize(splats["rotation"], dim=1)
        w, x, y, z = q.unbind(1)
        R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                         2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)
        M = R * scales[:, None, :]
        covars = torch.bmm(M, M.transpose(1, 2))
        gate = 1.0 / (1.0 + torch.exp(-100.0 * ((1.0 - o) - 0.995)))
        noise = torch.randn(splats["means"].shape, generator=generator, device=o.device) * gate[:, None] * (lr * cfg.noise_lr)
        splats["means"].add_(torch.einsum("bij,bj->bi", covars, noise))


def relocation_table(dev):
    """coef[r - 1, k] = sum_{i = k + 1 .. r} C(i - 1, k) (-1)^k / sqrt(k + 1): D(o', r) = sum_k coef[r - 1, k] o'^(k + 1)."""
    coef = torch.zeros(51, 51, dtype=torch.float64)
    for r in range(1, 52):
        for k in range(r):
            coef[r - 1, k] = sum(math.comb(i - 1, k) for i in range(k + 1, r + 1)) * (-1.0) ** k / math.sqrt(k + 1)
    return coef.float().to(dev)


def torch_update(tables, idx, n, cfg, coef):
    o, s = torch.sigmoid(tables["opacity"][idx]), torch.exp(tables["scaling"][idx])
    ratio = (torch.bincount(idx, minlength=n)[idx] + 1).clamp(1, 51)
    on = 1.0 - torch.pow(1.0 - o, 1.0 / ratio)
    powers = on[:, None] ** torch.arange(1, 52, device=o.device)
    denom = (coef[ratio - 1] * powers).sum(dim=1)
    on = on.clamp(cfg.min_opacity, 1.0 - torch.finfo(torch.float32).eps)
    tables["opacity"][idx] = torch.logit(on)
    tables["scaling"][idx] = torch.log(s * (o / denom)[:, None])


def round_torch(tables, moments, cfg, coef, n_new):
    """relocate, then sample_add, as gsplat runs them."""
    n = tables["opacity"].shape[0]
    o = torch.sigmoid(tables["opacity"])
    dead = o <= cfg.min_opacity
    dead_idx, alive_idx = torch.where(dead)[0], torch.where(~dead)[0]
    if len(dead_idx):
        sampled = alive_idx[torch.multinomial(o[alive_idx], len(dead_idx), replacement=True)]
        torch_update(tables, sampled, n, cfg, coef)
        for k, v in tables.items():
            v[dead_idx] = v[sampled]
        for ms in moments.values():
            for m in ms:
                m[sampled] = 0
    sampled = torch.multinomial(torch.sigmoid(tables["opacity"]), n_new, replacement=True)
    torch_update(tables, sampled, n, cfg, coef)
    tables = {k: torch.cat([v, v[sampled]]) for k, v in tables.items()}
    out = {}
    for k, ms in moments.items():
        for m in ms:
            m[sampled] = 0
        out[k] = [torch.cat([m, torch.zeros((n_new,) + tuple(m.shape[1:]), device=m.device)]) for m in ms]
    return tables, out, len(dead_idx)


def growth(dev, name="T1", steps=200):
    """PSNR after `steps` steps from every second Gaussian of a seeded scene under the MCMC strategy, the default one and with the set
    fixed.  Recorded, not asserted."""
    cfg = syn.CONFIGS[name]
    full = make_splats(cfg, dev, degree=0)
    K, vms = syn.intrinsics(cfg).to(dev), syn.make_cameras(cfg).to(dev)
    with torch.no_grad():
        images = [render_splats(full, vms[v], K, cfg.width, cfg.height).clamp(0.0, 1.0) for v in range(vms.shape[0])]
    start = {k: t[::2].contiguous() for k, t in full.items()}
    score = lambda s: gsbp_amd.score_image_views(s, vms, K, cfg.width, cfg.height, lambda v: images[v])["mean"]["psnr"]  # noqa: E731
    run = lambda **kw: gsbp_amd.train_scene(start, vms, K, cfg.width, cfg.height, lambda v: images[v], steps, **kw)  # noqa: E731
    n0 = start["means"].shape[0]
    mc, hist = run(strategy=gsbp_amd.MCMCConfig(refine_start_iter=20, refine_every=20, cap_max=2 * n0), opacity_reg=0.01, scale_reg=0.01)
    df, _ = run(strategy=gsbp_amd.DensifyConfig(refine_start_iter=20, refine_every=20, grow_scale3d=cfg.log_scale0,
                                                prune_scale3d=10 * cfg.log_scale0))
    fixed, _ = gsbp_amd.polish_scene(start, vms, K, cfg.width, cfg.height, lambda v: images[v], params=tuple(PARAM_KEYS), steps=steps)
    return dict(config=name, steps=steps, n_start=n0, n_mcmc=mc["means"].shape[0], n_default=df["means"].shape[0], rounds=len(hist["rounds"]),
                relocated=sum(r["relocated"] for r in hist["rounds"]), psnr_start=round(score(start), 3), psnr_mcmc=round(score(mc), 3),
                psnr_default=round(score(df), 3), psnr_fixed=round(score(fixed), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--repeats", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_mcmc.py measures on a GPU; there is nothing to report without one")
    dev = torch.device("cuda:0")
    cfg = syn.CONFIGS[a.config]
    W, H = cfg.width, cfg.height
    K, vms = syn.intrinsics(cfg).to(dev), syn.make_cameras(cfg, n_views=2).to(dev)
    full = make_splats(cfg, dev)
    n = full["means"].shape[0]
    with torch.no_grad():
        images = [render_splats(full, vms[v], K, W, H).clamp(0.0, 1.0) for v in range(2)]
    gen = torch.Generator().manual_seed(11)
    work = {k: (t + 0.01 * torch.randn(t.shape, generator=gen).to(dev)).requires_grad_(True) for k, t in full.items()}
    opt = optimizer_of(work)
    mcfg = gsbp_amd.MCMCConfig(cap_max=2 * n)
    lr = opt.param_groups[0]["lr"]
    noise_gen = torch.Generator(device=dev).manual_seed(5)

    def step(form, v):
        opt.zero_grad(set_to_none=True)
        loss = gsbp_amd.photometric_loss(render_splats(work, vms[v], K, W, H), images[v])
        if form != "step_fixed":
            loss = loss + 0.01 * torch.sigmoid(work["opacity"]).mean() + 0.01 * torch.exp(work["scaling"]).mean()
        loss.backward()
        opt.step()
        if form == "step_mcmc":
            gsbp_amd.inject_noise(work, lr, mcfg, generator=noise_gen)
        elif form == "step_noise_torch":
            noise_torch(work, lr, mcfg, generator=noise_gen)

    names = ("step_fixed", "step_mcmc", "step_noise_torch", "noise_kernel", "noise_torch", "round_kernels", "round_torch")
    ms = {k: [] for k in names}
    peak = {k: 0.0 for k in names}

    def record(name, rep, t, p):
        if rep >= a.warmup:
            ms[name].append(t)
            peak[name] = max(peak[name], p)

    for rep in range(a.repeats + a.warmup):
        for name in ("step_fixed", "step_mcmc", "step_noise_torch"):
            _, t, p = timed(lambda: step(name, rep % 2))
            record(name, rep, t, p)
    # the noise alone, on a copy with a learning rate of zero weight on the outcome: both forms draw and write, nothing accumulates
    still = {k: work[k].detach().clone() for k in ("means", "scaling", "rotation", "opacity")}
    for rep in range(a.repeats + a.warmup):
        for name, fn in (("noise_kernel", gsbp_amd.inject_noise), ("noise_torch", noise_torch)):
            _, t, p = timed(lambda: fn(still, 1e-12, mcfg, generator=noise_gen))
            record(name, rep, t, p)
    # one relocate + add round with about 15 % dead, both forms on copies of the same parameters and moments
    coef = relocation_table(dev)
    dead = torch.rand(n, generator=torch.Generator().manual_seed(3)).to(dev) < 0.15
    sizes, moved = {}, {}
    for rep in range(a.repeats + a.warmup):
        for name in ("round_kernels", "round_torch"):
            params = {k: work[k].detach().clone() for k in KEYS}
            params["opacity"][dead] = -7.0
            params = {k: v.requires_grad_(True) for k, v in params.items()}
            o = optimizer_of(params)
            for k in KEYS:
                o.state[params[k]] = {kk: vv.clone() for kk, vv in opt.state[work[k]].items()}
            if name == "round_kernels":
                def kernels():
                    p1, i1 = gsbp_amd.relocate(params, mcfg, optimizer=o, generator=noise_gen)
                    return gsbp_amd.sample_add(p1, mcfg, mcfg.n_new(n), optimizer=o, generator=noise_gen), i1
                ((new, info), i1), t, p = timed(kernels)
                sizes[name], moved[name] = info["n_after"], i1["relocated"]
            else:
                tables = {k: params[k].detach() for k in KEYS}
                moments = {k: [o.state[params[k]]["exp_avg"], o.state[params[k]]["exp_avg_sq"]] for k in KEYS}
                (new, _, n_dead), t, p = timed(lambda: round_torch(tables, moments, mcfg, coef, mcfg.n_new(n)))
                sizes[name], moved[name] = new["means"].shape[0], n_dead
            record(name, rep, t, p)
            del new, params, o
    assert sizes["round_kernels"] == sizes["round_torch"] and moved["round_kernels"] == moved["round_torch"], (sizes, moved)
    timing = dict(tool="tools/time_mcmc.py", device=torch.cuda.get_device_name(0), date=time.strftime("%Y-%m-%d"), config=a.config,
                  n_gaussians=n, width=W, height=H, sh_degree=3, repeats=a.repeats, warmup=a.warmup,
                  round=dict(relocated=moved["round_kernels"], n_after=sizes["round_kernels"]), forms={})
    for name, ts in ms.items():
        timing["forms"][name] = dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4),
                                     peak_mib=round(peak[name], 1))
        print(name, json.dumps(timing["forms"][name]), flush=True)
    f = timing["forms"]
    timing["step_mcmc_over_step_fixed"] = round(f["step_mcmc"]["median_ms"] / f["step_fixed"]["median_ms"], 4)
    timing["step_noise_torch_over_step_mcmc"] = round(f["step_noise_torch"]["median_ms"] / f["step_mcmc"]["median_ms"], 4)
    timing["noise_torch_over_noise_kernel"] = round(f["noise_torch"]["median_ms"] / f["noise_kernel"]["median_ms"], 3)
    timing["round_torch_over_round_kernels"] = round(f["round_torch"]["median_ms"] / f["round_kernels"]["median_ms"], 3)
    del work, opt, full, images, still
    torch.cuda.empty_cache()
    timing["growth"] = growth(dev)
    print("timing", json.dumps({k: v for k, v in timing.items() if k != "forms"}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(timing, fh, indent=1)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
