"""The yardstick of the fused Adam step (csrc/adam_math.h, csrc/adam.hip).

`chain32` is adam_math.h in numpy float32, expression for expression: it gives the header's BITS (host program and kernel alike), as
mcmc_ref.py does for its header.  `chain64` is the same chain in float64 with the float64 scalars: the truth.  A float32 result that is
not bit-comparable (torch.optim.Adam's, whose lerp and addcmul may fuse) is held against the truth by the project's floor rule, per
tensor and figure (Frobenius norm, max-abs):

    figure(got - truth) <= FACTOR x max(figure(floor - truth), 2^-24 x figure(truth))

with torch's own float32 result as the floor.

Denormals are not pinned: make_tables draws inputs under which every intermediate of the chain is a normal number or zero
(check_normal says so), because the device's and numpy's treatment of float32 denormals is not part of the contract.
"""
import numpy as np

F = np.float32
B1, B2, EPS = 0.9, 0.999, 1e-15  # the trainer's: torch's betas, the reference trainer's eps
TENSORS = ("p", "m", "v")
FIGURES = ("fro", "max")
TINY = float(np.finfo(np.float32).tiny)


def scalars64(step, lr, b1=B1, b2=B2):
    """(lr / (1 - b1^t), sqrt(1 - b2^t)) in float64, as torch's single-tensor Adam and engine.adam_scalars form them."""
    return float(lr) / (1.0 - float(b1) ** int(step)), (1.0 - float(b2) ** int(step)) ** 0.5


def scalars32(step, lr, b1=B1, b2=B2, eps=EPS):
    """AdamScalars::make: every scalar computed in float64 and rounded to float32 once."""
    step_size, sqrt_bc2 = scalars64(step, lr, b1, b2)
    return dict(step_size=F(step_size), sqrt_bc2=F(sqrt_bc2), one_minus_b1=F(1.0 - b1), b2=F(b2), one_minus_b2=F(1.0 - b2), eps=F(eps))


def chain32(p, g, m, v, step, lr, b1=B1, b2=B2, eps=EPS, mutant=None, want_parts=False):
    """(p', m', v') of adam_element on float32 arrays, in the header's order.  mutant: None | "no_bias_correction" | "eps_in_sqrt" |
    "b2_for_m" -- what a comparison must catch."""
    p, g, m, v = (np.asarray(a, F) for a in (p, g, m, v))
    S = scalars32(step, lr, b1, b2, eps)
    if mutant == "no_bias_correction":
        S["step_size"], S["sqrt_bc2"] = F(lr), F(1.0)
    if mutant == "b2_for_m":
        S["one_minus_b1"] = S["one_minus_b2"]
    with np.errstate(all="ignore"):
        d = g - m
        m1 = m + S["one_minus_b1"] * d
        t = S["one_minus_b2"] * g
        v1 = S["b2"] * v + t * g
        if mutant == "eps_in_sqrt":
            denom = np.sqrt(v1 + S["eps"]) / S["sqrt_bc2"]
        else:
            denom = np.sqrt(v1) / S["sqrt_bc2"] + S["eps"]
        q = m1 / denom
        u = S["step_size"] * q
        p1 = p - u
    out = tuple(np.ascontiguousarray(a, F) for a in (p1, m1, v1))
    if want_parts:
        return out, dict(d=d, c1d=S["one_minus_b1"] * d, m1=m1, t=t, tg=t * g, b2v=S["b2"] * v, v1=v1, root=np.sqrt(v1), denom=denom, q=q,
                         u=u, p1=p1)
    return out


def chain64(p, g, m, v, step, lr, b1=B1, b2=B2, eps=EPS):
    """The same chain in float64 with float64 scalars: the truth."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    step_size, sqrt_bc2 = scalars64(step, lr, b1, b2)
    m1 = m + (1.0 - b1) * (g - m)
    v1 = b2 * v + ((1.0 - b2) * g) * g
    p1 = p - step_size * (m1 / (np.sqrt(v1) / sqrt_bc2 + eps))
    return p1, m1, v1


def masked32(p, g, m, v, visible, step, lr, **kw):
    """chain32 on the rows with visible != 0 of [n, w] tables; every other row keeps its bits."""
    p, g, m, v = (np.asarray(a, F) for a in (p, g, m, v))
    fresh = chain32(p, g, m, v, step, lr, **kw)
    if visible is None:
        return fresh
    keep = np.asarray(visible).astype(bool)
    out = []
    for old, new in zip((p, m, v), fresh):
        res = old.copy()
        res[keep] = new[keep]
        out.append(res)
    return tuple(out)


def run_steps(chain, p, m, v, grads, lr, first_step=1, **kw):
    """`chain` applied once per gradient of `grads`, the step count rising from first_step."""
    for i, g in enumerate(grads):
        p, m, v = chain(p, g, m, v, first_step + i, lr, **kw)
    return dict(p=p, m=m, v=v)


def signed_log_uniform(rng, shape, lo, hi):
    return (rng.choice([-1.0, 1.0], size=shape) * np.exp(rng.uniform(np.log(lo), np.log(hi), size=shape))).astype(F)


def make_tables(n, w, seed=0, zero_moments=False):
    """dict(p, g, m, v) float32 [n, w]: gradient magnitudes log-uniform in [1e-12, 1e2] with one element in eight an exact zero (of
    either sign); moments zero (zero_moments, and one row in four otherwise) or non-zero, m of either sign in [1e-10, 1e1], v in
    [1e-20, 1e2]."""
    r = np.random.default_rng(7919 * seed + 131 * n + w)
    p = r.normal(size=(n, w)).astype(F)
    g = signed_log_uniform(r, (n, w), 1e-12, 1e2)
    zero = r.random((n, w)) < 0.125
    g[zero] = np.where(r.random((n, w)) < 0.5, F(0.0), F(-0.0))[zero]
    m = signed_log_uniform(r, (n, w), 1e-10, 1e1)
    v = np.abs(signed_log_uniform(r, (n, w), 1e-20, 1e2))
    fresh = np.ones(n, bool) if zero_moments else (np.arange(n) % 4 == 3)
    m[fresh], v[fresh] = 0.0, 0.0
    return dict(p=p, g=g, m=m, v=v)


def check_normal(parts):
    """Every intermediate of chain32 is a normal float32 or zero (and finite)."""
    for name, a in parts.items():
        a = np.abs(np.asarray(a, np.float64))
        assert np.isfinite(a).all(), name
        assert ((a == 0) | (a >= TINY)).all(), (name, a[(a != 0) & (a < TINY)][:4])


def masks(n, seed=0):
    """The masks of the tests: name -> None or uint8 [n]."""
    r = np.random.default_rng(977 * seed + n)
    one_hot = lambda i: (np.arange(n) == i).astype(np.uint8)  # noqa: E731
    return {"none": None, "ones": np.ones(n, np.uint8), "zeros": np.zeros(n, np.uint8), "alternating": (np.arange(n) % 2).astype(np.uint8),
            "row0": one_hot(0), "last": one_hot(n - 1), "random": (r.permutation(n) < (n + 1) // 2).astype(np.uint8)}


def figures(a):
    a = np.asarray(a, np.float64)
    return dict(fro=float(np.linalg.norm(a)), max=float(np.abs(a).max()) if a.size else 0.0)


def ratios(got, truth, floor):
    """{(tensor, figure): figure(got - truth) / max(figure(floor - truth), 2^-24 figure(truth))} over p, m, v; a truth of all zeros
    admits nothing: 0 where got is all zeros too, inf otherwise."""
    out = {}
    for name in TENSORS:
        g, t, f = (np.asarray(x[name], np.float64) for x in (got, truth, floor))
        eg, ef, ft = figures(g - t), figures(f - t), figures(t)
        for fig in FIGURES:
            bound = max(ef[fig], 2.0 ** -24 * ft[fig])
            out[(name, fig)] = 0.0 if eg[fig] == 0.0 else (eg[fig] / bound if bound > 0.0 else float("inf"))
    return out


def torch_adam(p, grads, lr, device="cpu", b1=B1, b2=B2, eps=EPS, **adam_kw):
    """dict(p, m, v) after torch.optim.Adam has stepped a float32 copy of p once per gradient: the floor."""
    import torch
    q = torch.from_numpy(np.array(p, F)).to(device).requires_grad_(True)  # (a copy: the steps are in place)
    opt = torch.optim.Adam([q], lr=lr, betas=(b1, b2), eps=eps, **adam_kw)
    for g in grads:
        q.grad = torch.from_numpy(np.ascontiguousarray(g, F)).to(device)
        opt.step()
    st = opt.state[q]
    return dict(p=q.detach().cpu().numpy(), m=st["exp_avg"].cpu().numpy(), v=st["exp_avg_sq"].cpu().numpy())
