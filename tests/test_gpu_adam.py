"""The fused Adam step on the device (csrc/adam.hip): the kernel against the numpy float32 restatement of adam_math.h
(tests/adam_ref.py) BIT FOR BIT over the widths, sizes and masks below -- invisible rows and the guard rows around the table keep every
bit, also where 16-B chunks straddle rows (w = 1, 3, 45); SplatAdam against torch.optim.Adam on the device by the floor rule with the
float64 chain as the truth; its state layout; and a densify round and an MCMC relocate + add round that carry a SplatAdam's moments
exactly as they carry torch's.

Denormal behaviour is NOT pinned: adam_ref.make_tables draws inputs under which every intermediate is a normal number or zero (checked
here per shape), because the device's and numpy's float32 denormal modes are not part of the contract.

DEVICE_FACTOR.  SplatAdam and torch's multi-tensor Adam on the device are the same expressions up to fused multiply-adds and the order
in which the step size enters.  Measured on an MI355X over the seven tables x 1 and 25 steps x 3 tensors x 2 figures (the test prints
its largest): ratios 0.273 .. 2.127, the largest on the max-abs figure of exp_avg_sq of the [N, 3] means table after one step (there
v' = ((1 - b2) g) g here and (1 - b2) (g g) there: one rounding each, on either side of the truth); DEVICE_FACTOR = ceil(2 x 2.127) = 5.
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import adam_ref as ref
import gsbp_amd
from gsbp_amd import _lib
from gsbp_amd._lib import ptr
from gsbp_amd.engine import adam_step_tables
from gsbp_amd.sh import device_caller
from test_gpu_densify import probe_thresholds, t0_training_setup
from test_gpu_mcmc import finite_scene, up
from test_mcmc_cpu import same_bits

pytestmark = pytest.mark.gpu
DEVICE_FACTOR = 5.0
LR, STEP = 1e-2, 3
GUARD = 4  # rows in front of and behind the table: 4 w floats keep the table 16-B aligned for every w


def guarded(a, dev, seed):
    """(buffer [GUARD + n + GUARD, w] on the device with seeded rows around `a`, the table's view of it, the buffer's host copy)."""
    n, w = a.shape
    host = np.random.default_rng(seed).normal(size=(n + 2 * GUARD, w)).astype(np.float32)
    host[GUARD:GUARD + n] = a
    buf = torch.from_numpy(host).to(dev)
    table = buf[GUARD:GUARD + n]
    assert table.is_contiguous() and table.data_ptr() % 16 == 0
    return buf, table, host


def run_kernel(dev, t, visible, step=STEP, lr=LR):
    """The kernel on guarded copies of t's tables: (dict of the three buffers' host copies after, the same before, g after)."""
    bufs = {k: guarded(t[k], dev, seed=i) for i, k in enumerate(("p", "g", "m", "v"))}
    vis = None if visible is None else torch.from_numpy(visible).to(dev)
    call, stream = device_caller(dev)
    adam_step_tables(call, stream, bufs["p"][1], bufs["g"][1], bufs["m"][1], bufs["v"][1], vis, step, lr, ref.B1, ref.B2, ref.EPS)
    return {k: bufs[k][0].cpu().numpy() for k in bufs}, {k: bufs[k][2] for k in bufs}


@pytest.mark.parametrize("n", [1, 5, 257, 1025])
@pytest.mark.parametrize("w", [1, 3, 4, 45, 128])
def test_kernel_bit_for_bit_under_every_mask(dev, w, n):
    for zero_moments in (False, True):
        t = ref.make_tables(n, w, seed=int(zero_moments), zero_moments=zero_moments)
        ref.check_normal(ref.chain32(t["p"], t["g"], t["m"], t["v"], STEP, LR, want_parts=True)[1])
        for name, visible in ref.masks(n, seed=w).items():
            after, before = run_kernel(dev, t, visible)
            want = dict(zip(("p", "m", "v"), ref.masked32(t["p"], t["g"], t["m"], t["v"], visible, STEP, LR)))
            for k in ("p", "m", "v"):
                got = after[k][GUARD:GUARD + n]
                assert same_bits(got, want[k]), (name, zero_moments, k, int((got.view(np.uint32) != want[k].view(np.uint32)).sum()))
                if visible is not None:  # invisible rows: the bits they had (the restatement says so too; this says it of the device)
                    assert same_bits(got[visible == 0], t[k][visible == 0]), (name, k)
                assert same_bits(after[k][:GUARD], before[k][:GUARD]) and same_bits(after[k][GUARD + n:], before[k][GUARD + n:]), (name, k)
            assert same_bits(after["g"], before["g"]), name
            if name in ("ones", "none"):
                assert (after["p"][GUARD:GUARD + n] != t["p"]).any()


def test_two_runs_give_the_same_bytes_and_the_engine_method_is_the_same_kernel(dev):
    t = ref.make_tables(1025, 45, seed=4)
    visible = ref.masks(1025, seed=4)["random"]
    a, _ = run_kernel(dev, t, visible)
    b, _ = run_kernel(dev, t, visible)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)
    eng = gsbp_amd.Engine(16, 16, 16, device=dev)
    tabs = {k: up(t[k], dev) for k in t}
    eng.adam_step(tabs["p"], tabs["g"], tabs["m"], tabs["v"], STEP, LR, ref.B1, ref.B2, ref.EPS, visible=up(visible, dev).bool())
    for k in ("p", "m", "v"):
        assert same_bits(tabs[k].cpu().numpy(), a[k][GUARD:GUARD + 1025]), k


def test_no_rows_is_a_no_op(dev):
    buf = torch.arange(64, dtype=torch.float32, device=dev)
    keep = buf.clone()
    rc = _lib.lib().gwbp_adam_step(0, 3, ptr(buf), ptr(buf[16:]), ptr(buf[32:]), ptr(buf[48:]), None, 1e-3, 0.5, 0.9, 0.999, 1e-15,
                                   C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0
    empty = torch.zeros(0, 3, device=dev)
    call, stream = device_caller(dev)
    adam_step_tables(call, stream, empty, empty.clone(), empty.clone(), empty.clone(), None, 1, LR, ref.B1, ref.B2, ref.EPS)
    torch.cuda.synchronize(dev)
    assert torch.equal(buf, keep)


# ---- SplatAdam ------------------------------------------------------------------------------------------------------------------------
TABLES = dict(means=(3,), scaling=(3,), rotation=(4,), opacity=(), features_dc=(1, 3), features_rest=(15, 3), features=(128,))
LRS = dict(means=1.6e-4, scaling=5e-3, rotation=1e-3, opacity=5e-2, features_dc=2.5e-3, features_rest=2.5e-3 / 20, features=2.5e-3)
N_T0 = 512


@pytest.fixture(scope="module")
def sequences():
    """Per table of T0's size: the start, 25 gradients, and the float64 truth after 1 and 25 steps, computed once on the CPU."""
    out = {}
    for i, (key, tail) in enumerate(TABLES.items()):
        w = int(np.prod(tail, dtype=np.int64))
        p = ref.make_tables(N_T0, w, seed=20 + i)["p"].reshape((N_T0,) + tail)
        grads = [ref.make_tables(N_T0, w, seed=1000 + 31 * i + s)["g"].reshape((N_T0,) + tail) for s in range(25)]
        zero = np.zeros_like(p)
        truth = {steps: ref.run_steps(ref.chain64, p, zero, zero, grads[:steps], LRS[key]) for steps in (1, 25)}
        out[key] = dict(p=p, grads=grads, truth=truth)
    return out


def groups_of(seq, dev):
    params = {k: up(s["p"].copy(), dev).requires_grad_(True) for k, s in seq.items()}
    return params, [dict(params=[params[k]], lr=LRS[k]) for k in seq]


def results(opt, params):
    return {k: dict(p=p.detach().cpu().numpy(), m=opt.state[p]["exp_avg"].cpu().numpy(), v=opt.state[p]["exp_avg_sq"].cpu().numpy())
            for k, p in params.items()}


def test_splat_adam_against_torch_adam_by_the_floor_rule(dev, sequences):
    runs = {}
    for name, cls in (("splat", gsbp_amd.SplatAdam), ("torch", torch.optim.Adam)):
        params, groups = groups_of(sequences, dev)
        opt = cls(groups, eps=ref.EPS)
        for s in range(25):
            for k, p in params.items():
                p.grad = up(sequences[k]["grads"][s], dev)
            opt.step()
            if s + 1 in (1, 25):
                runs[(name, s + 1)] = results(opt, params)
        runs[name] = (opt, params)
    lo, hi = float("inf"), 0.0
    for steps in (1, 25):
        for k in TABLES:
            r = ref.ratios(runs[("splat", steps)][k], sequences[k]["truth"][steps], runs[("torch", steps)][k])
            worst = max(r, key=r.get)
            print(f"{k}, {steps} steps: SplatAdam / floor, largest {r[worst]:.3f} at {worst}")
            lo, hi = min(lo, min(r.values())), max(hi, r[worst])
            assert r[worst] <= DEVICE_FACTOR, (k, steps, r)
    print(f"SplatAdam / floor over every table: {lo:.3f} .. {hi:.3f}")
    # the state's layout is torch's: keys, types, dtypes, shapes, devices -- the count a host scalar
    (ours, ours_p), (theirs, theirs_p) = runs["splat"], runs["torch"]
    for k in TABLES:
        a, b = ours.state[ours_p[k]], theirs.state[theirs_p[k]]
        assert list(a) == list(b) == ["step", "exp_avg", "exp_avg_sq"]
        for name in a:
            assert type(a[name]) is type(b[name]) and a[name].dtype == b[name].dtype and a[name].shape == b[name].shape, (k, name)
            assert a[name].device == b[name].device, (k, name)
        assert a["step"].device.type == "cpu" and float(a["step"]) == float(b["step"]) == 25.0
    sd = ours.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and len(sd["param_groups"]) == len(TABLES)


def test_splat_adam_masks_skips_and_refusals(dev):
    n = 300
    p, q = torch.randn(n, 3, device=dev).requires_grad_(True), torch.randn(n, device=dev).requires_grad_(True)
    dec = torch.randn(7, 5, device=dev).requires_grad_(True)
    idle = torch.randn(n, 2, device=dev).requires_grad_(True)
    opt = gsbp_amd.SplatAdam([dict(params=[p], lr=0.1), dict(params=[q], lr=0.2), dict(params=[dec], lr=0.3), dict(params=[idle], lr=0.1)])
    before = {k: t.detach().clone() for k, t in (("p", p), ("q", q), ("dec", dec), ("idle", idle))}
    p.grad = torch.ones(n, 1, device=dev).expand(n, 3)  # not contiguous: made so
    q.grad, dec.grad = torch.ones(n, device=dev), torch.ones(7, 5, device=dev)
    assert not p.grad.is_contiguous()
    radii = torch.zeros(2, n, dtype=torch.int32, device=dev)
    radii[0, :100], radii[1, 50:150] = 3, 1
    with pytest.raises(gsbp_amd.GwbpError, match="dense="):
        opt.step(visible=radii)                      # the decoder has 7 rows
    assert len(opt.state) == 0 and torch.equal(p.detach(), before["p"])  # a call that raises has stepped nothing
    opt.step(visible=radii, dense=[dec])
    seen = torch.arange(n, device=dev) < 150
    for t, old in ((p, before["p"]), (q, before["q"])):
        assert torch.equal(t.detach()[~seen], old[~seen]) and bool((t.detach()[seen] != old[seen]).all())
        assert not opt.state[t]["exp_avg"][~seen].any() and bool(opt.state[t]["exp_avg"][seen].all())
    assert bool((dec.detach() != before["dec"]).all()) and torch.equal(idle.detach(), before["idle"]) and idle not in opt.state
    assert float(opt.state[p]["step"]) == float(opt.state[dec]["step"]) == 1.0
    # a mask of zeros moves nothing, and the count still advances
    now = p.detach().clone()
    opt.step(visible=torch.zeros(n, dtype=torch.bool, device=dev), dense=[dec])
    assert torch.equal(p.detach(), now) and float(opt.state[p]["step"]) == 2.0
    opt.step(visible=torch.ones(n, dtype=torch.uint8, device=dev), dense=[dec])
    assert bool((p.detach() != now).all())
    for bad in (torch.ones(n + 1, dtype=torch.bool, device=dev), torch.ones(n, device=dev), torch.ones(n, dtype=torch.bool),
                torch.ones(2, n, dtype=torch.int64, device=dev)):
        with pytest.raises(gsbp_amd.GwbpError):
            opt.step(visible=bad, dense=[dec])
    p.grad = None
    opt.param_groups[0]["weight_decay"] = 0.1
    with pytest.raises(gsbp_amd.GwbpError, match="weight_decay"):
        opt.step()


# ---- the rounds carry a SplatAdam's moments as they carry torch's -----------------------------------------------------------------------
def twin(opt, params, keys, dev):
    """A SplatAdam over clones of `params` that holds the state of the torch.optim.Adam `opt` (its moments' bits, its counts)."""
    mine = {k: t.detach().clone().requires_grad_(True) for k, t in params.items()}
    ours = gsbp_amd.SplatAdam([dict(params=[mine[k]], lr=g["lr"]) for k, g in zip(keys, opt.param_groups)], eps=ref.EPS)
    ours.load_state_dict(copy.deepcopy(opt.state_dict()))  # (a copy: load_state_dict keeps the tensors it is handed)
    for k in keys:
        a, b = ours.state[mine[k]], opt.state[params[k]]
        assert a["exp_avg"] is not b["exp_avg"] and torch.equal(a["exp_avg"], b["exp_avg"]) and float(a["step"]) == float(b["step"])
        assert a["step"].device.type == "cpu"
    return mine, ours


def same_state(a_opt, a, b_opt, b, keys):
    for i, k in enumerate(keys):
        assert a_opt.param_groups[i]["params"][0] is a[k] and b_opt.param_groups[i]["params"][0] is b[k]
        assert torch.equal(a[k].detach(), b[k].detach()), k
        sa, sb = a_opt.state[a[k]], b_opt.state[b[k]]
        assert float(sa["step"]) == float(sb["step"])
        for name in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(sa[name], sb[name]) and bool(sa[name].any()), (k, name)
    assert len(a_opt.state) == len(b_opt.state) == len(keys)


def test_a_densify_round_moves_the_moments_as_under_torch_adam(dev):
    cfg, start, K, vms, images = t0_training_setup(dev)
    work, state, grow, opa = probe_thresholds(dev, start, K, vms, images, cfg)
    n = work["means"].shape[0]
    dcfg = gsbp_amd.DensifyConfig(grow_grad2d=grow, prune_opa=opa, grow_scale3d=0.06, prune_scale3d=0.25)
    keys = ("means", "scaling", "rotation", "opacity", "features_dc")
    params = {k: t.detach().clone().requires_grad_(True) for k, t in work.items()}
    opt = torch.optim.Adam([dict(params=[params[k]], lr=1e-3) for k in keys], eps=ref.EPS)
    gsbp_amd.photometric_loss(gsbp_amd.polish.render_splats(params, vms[0], K, cfg.width, cfg.height), images[0]).backward()
    opt.step()
    mine, ours = twin(opt, params, keys, dev)
    outs = []
    for p, o in ((params, opt), (mine, ours)):
        st = gsbp_amd.DensifyState(n, dev)
        st.grad2d, st.count = state.grad2d.clone(), state.count.clone()
        new, info = gsbp_amd.densify(p, st, dcfg, dcfg.reset_every + 100, optimizer=o, generator=torch.Generator(device=dev).manual_seed(77))
        outs.append((new, info))
    (new_t, info_t), (new_s, info_s) = outs
    assert info_t["n_after"] == info_s["n_after"] != n and min(info_s[k] for k in ("pruned", "kept", "cloned", "split")) > 0
    assert torch.equal(info_t["parent"], info_s["parent"])
    same_state(opt, new_t, ours, new_s, keys)
    gsbp_amd.reset_opacity(new_s, ours, dcfg)
    assert not ours.state[new_s["opacity"]]["exp_avg"].any()
    # ... and it steps the new leaves
    before = new_s["means"].detach().clone()
    image, meta = gsbp_amd.polish.render_splats(new_s, vms[1], K, cfg.width, cfg.height, return_meta=True, means2d_grad=True)
    gsbp_amd.photometric_loss(image, images[1]).backward()
    ours.step(visible=meta["radii"])
    assert float(ours.state[new_s["means"]]["step"]) == 2.0 and not torch.equal(new_s["means"].detach(), before)


def test_an_mcmc_relocate_and_add_round_moves_the_moments_as_under_torch_adam(dev):
    t = finite_scene()
    n = len(t["opacity"])
    keys = ("means", "scaling", "opacity")
    params = {k: up(v, dev).requires_grad_(True) for k, v in t.items() if k != "field"}
    opt = torch.optim.Adam([dict(params=[params[k]], lr=1e-3) for k in keys], eps=ref.EPS)
    sum((params[k] ** 2).sum() for k in keys).backward()
    opt.step()
    opt.zero_grad(set_to_none=True)
    mine, ours = twin(opt, params, keys, dev)
    mcfg = gsbp_amd.MCMCConfig(cap_max=n + 80)
    outs = []
    for p, o in ((params, opt), (mine, ours)):
        gen = torch.Generator(device=dev).manual_seed(77)
        moved, info = gsbp_amd.relocate(p, mcfg, optimizer=o, generator=gen)
        grown, added = gsbp_amd.sample_add(moved, mcfg, mcfg.n_new(n), optimizer=o, generator=gen)
        outs.append((grown, info, added))
    (new_t, info_t, added_t), (new_s, info_s, added_s) = outs
    assert info_s["relocated"] == info_t["relocated"] > 100 and added_s["added"] == added_t["added"] == 80
    assert torch.equal(info_t["parent"], info_s["parent"]) and torch.equal(added_t["parent"], added_s["parent"])
    same_state(opt, new_t, ours, new_s, keys)
    assert new_s["means"].shape[0] == n + 80 and not ours.state[new_s["means"]]["exp_avg"][n:].any()
    sum((new_s[k] ** 2).sum() for k in keys).backward()
    ours.step()
    assert float(ours.state[new_s["means"]]["step"]) == 2.0
