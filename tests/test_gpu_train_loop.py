"""polish_scene and train_scene (train.py) against the same loops written out here from public pieces -- trainable, view_schedule,
render_splats, photometric_loss and the strategies' public functions -- bit for bit: every returned tensor, the losses, the sizes, the
rounds and the resets.  What the comparison pins is the ORDER of a step (statistics before the rate decay, the optimiser before a
round, the reset behind the round) and the order in which the one device generator is consumed (split noise; relocate, sample_add,
inject_noise).

Every test runs on T0's training setup seen through the 32 x 16 centre crop of tests/test_gpu_train_adam.py: on two tiles training is
reproducible bit for bit (tests/test_gpu_mcmc.py, test_the_default_path_is_unchanged), so equal bits are what a correct loop gives and
any other order of the same calls is not.  256 Gaussians, at most 8 steps.
"""
import pytest
import torch

import gsbp_amd
from gsbp_amd.polish import PARAM_KEYS, means_group, means_lr_at, render_splats, table_sh_degree, trainable, view_schedule
from test_gpu_train_adam import CROP_H, CROP_W, crop  # noqa: F401  (the fixture)
from test_mcmc_cpu import same_bits

pytestmark = pytest.mark.gpu
SEED = 3
ROUND_KEYS = ("step", "n_before", "n_after", "pruned", "kept", "cloned", "split")


def read(losses):
    return torch.stack(losses).cpu().tolist()


def assert_same_tensors(got, want):
    assert sorted(got) == sorted(want)
    for k, t in want.items():
        assert not got[k].requires_grad and got[k].dtype == t.dtype, k
        assert same_bits(got[k].float().cpu().numpy(), t.detach().float().cpu().numpy()), k


def field_of(n, dev):
    return torch.randn(n, 3, generator=torch.Generator().manual_seed(5)).to(dev)


@pytest.mark.parametrize("adam", ["torch", "visible"])
def test_polish_scene_is_the_written_out_loop(dev, crop, adam):  # noqa: F811
    cfg, start, Kc, vms, crops = crop
    steps, interval, final = 4, 2, 0.01
    polished, losses = gsbp_amd.polish_scene(start, vms, Kc, CROP_W, CROP_H, lambda i: crops[i], params=tuple(PARAM_KEYS), steps=steps,
                                             seed=SEED, sh_degree_interval=interval, adam=adam, means_lr_final=final)
    work, opt = trainable(start, tuple(PARAM_KEYS), None, "polish_scene", adam)
    group, table = means_group(opt, work), table_sh_degree(work)
    lr0, want = group["lr"], []
    assert table == 1
    for step, v in enumerate(view_schedule(vms.shape[0], SEED, steps)):
        opt.zero_grad(set_to_none=True)
        image, meta = render_splats(work, vms[v], Kc, CROP_W, CROP_H, return_meta=True, means2d_grad=adam == "visible",
                                    sh_degree=min(step // interval, table))
        loss = gsbp_amd.photometric_loss(image, crops[v])
        loss.backward()
        group["lr"] = means_lr_at(lr0, final, step, steps)
        if adam == "visible":
            opt.step(visible=meta["radii"])
        else:
            opt.step()
        want.append(loss.detach())
    assert losses == read(want) and len(set(losses)) == steps
    assert_same_tensors(polished, work)
    assert not torch.equal(polished["features_rest"], start["features_rest"])  # (degree 1 was reached, and trained)


def test_train_scene_default_strategy_is_the_written_out_loop(dev, crop):  # noqa: F811
    cfg, start, Kc, vms, crops = crop
    dcfg = gsbp_amd.DensifyConfig(refine_start_iter=1, refine_every=2, reset_every=4, refine_stop_iter=7, max_gaussians=512)
    n0, steps = start["means"].shape[0], 8
    trained, hist = gsbp_amd.train_scene(start, vms, Kc, CROP_W, CROP_H, lambda i: crops[i], steps, seed=SEED, strategy=dcfg,
                                         carry=dict(field=field_of(n0, dev)))
    work, opt = trainable(start, tuple(PARAM_KEYS), None, "train_scene")
    state, gen = gsbp_amd.DensifyState(n0, dev), torch.Generator(device=dev).manual_seed(SEED)
    carried, want, sizes, rounds, resets = dict(field=field_of(n0, dev)), [], [], [], []
    for step, v in enumerate(view_schedule(vms.shape[0], SEED, steps)):
        opt.zero_grad(set_to_none=True)
        image, meta = render_splats(work, vms[v], Kc, CROP_W, CROP_H, return_meta=True, means2d_grad=True)
        loss = gsbp_amd.photometric_loss(image, crops[v])
        loss.backward()
        if step < dcfg.refine_stop_iter:
            state.update(meta)
        opt.step()
        want.append(loss.detach())
        sizes.append(int(work["means"].shape[0]))
        if dcfg.refines_at(step):
            work, info = gsbp_amd.densify(work, state, dcfg, step, optimizer=opt, carry=carried, generator=gen)
            carried = info["carry"]
            rounds.append({k: info[k] for k in ROUND_KEYS})
        if dcfg.resets_at(step):
            gsbp_amd.reset_opacity(work, opt, dcfg)
            resets.append(step)
    assert [r["step"] for r in rounds] == [2, 4, 6] and resets == [4] and any(r["n_after"] != r["n_before"] for r in rounds)
    assert hist["loss"] == read(want) and hist["n"] == sizes and hist["rounds"] == rounds and hist["resets"] == resets
    assert hist["sh_degree"] == [1] * steps and "means_lr" not in hist
    assert_same_tensors(trained, work)
    assert_same_tensors(hist["carry"], carried)


def test_train_scene_mcmc_is_the_written_out_loop(dev, crop):  # noqa: F811
    cfg, start, Kc, vms, crops = crop
    mcfg = gsbp_amd.MCMCConfig(refine_start_iter=1, refine_every=2, cap_max=290)
    n0, steps, reg = start["means"].shape[0], 6, 0.01
    trained, hist = gsbp_amd.train_scene(start, vms, Kc, CROP_W, CROP_H, lambda i: crops[i], steps, seed=SEED, strategy=mcfg,
                                         opacity_reg=reg, scale_reg=reg, carry=dict(field=field_of(n0, dev)))
    work, opt = trainable(start, tuple(PARAM_KEYS), None, "train_scene")
    gen = torch.Generator(device=dev).manual_seed(SEED)  # ONE generator: relocate, sample_add, inject_noise draw from it in that order
    carried, want, sizes, rounds = dict(field=field_of(n0, dev)), [], [], []
    for step, v in enumerate(view_schedule(vms.shape[0], SEED, steps)):
        opt.zero_grad(set_to_none=True)
        image = render_splats(work, vms[v], Kc, CROP_W, CROP_H)
        loss = gsbp_amd.photometric_loss(image, crops[v])
        loss = loss + reg * torch.sigmoid(work["opacity"]).mean()
        loss = loss + reg * torch.exp(work["scaling"]).mean()
        loss.backward()
        opt.step()
        want.append(loss.detach())
        sizes.append(int(work["means"].shape[0]))
        if mcfg.refines_at(step):
            work, moved = gsbp_amd.relocate(work, mcfg, optimizer=opt, carry=carried, generator=gen)
            work, added = gsbp_amd.sample_add(work, mcfg, mcfg.n_new(sizes[-1]), optimizer=opt, carry=moved["carry"], generator=gen)
            carried = added["carry"]
            rounds.append(dict(step=step, n_before=sizes[-1], n_after=added["n_after"], relocated=moved["relocated"], added=added["added"]))
        gsbp_amd.inject_noise(work, means_group(opt, work)["lr"], mcfg, generator=gen)
    assert [r["step"] for r in rounds] == [2, 4] and [r["added"] for r in rounds] == [12, 13] and sizes[-1] == 281
    assert hist["loss"] == read(want) and hist["n"] == sizes and hist["rounds"] == rounds and hist["resets"] == []
    assert_same_tensors(trained, work)
    assert_same_tensors(hist["carry"], carried)
