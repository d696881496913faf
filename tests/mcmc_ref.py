"""The yardstick of the MCMC strategy (csrc/mcmc.hip, csrc/mcmc_math.h) in numpy.

Two restatements:

  * the FUSED rule as the kernels run it, in float32 and in the documented operation order, with int64 prefix sums and
    np.searchsorted for the index logic -- plan, draw, update, move, zero_rows, noise.  The build forbids contraction and rounds divide
    and sqrt correctly, and numpy's float32 ufuncs round each operation once, so this gives the kernels' bits EXCEPT at the library
    calls: expf and logf of the activations and the one powf.  Every function that reaches one takes `lib`, an object with exp(a),
    log(a) and pow(a, b) on float32 arrays: ONCE (the float64 function rounded once) is the restatement's own; a test hands in the
    host's libm or the device's (gwbp_mcmc_libm) and then holds the bits.
  * gsplat's LITERAL rule in float64 -- literal_relocate, literal_sample_add, literal_compute_relocation with pow and exact
    binomials, literal_inject_noise through M = R S, M M^T.  They take the draws as given parents; literal_parents is the
    inverse-CDF draw over the exact float64 probabilities of the Gaussians the rule samples from.

relocation_bounds and noise_bound say how far the float32 fused form may lie from the float64 literal one on the same float32
inputs; their derivations stand beside them (and in DESIGN.md 4.0j).  `mutant` arguments build deliberately wrong variants;
tests/test_mcmc_cpu.py shows that each of them is caught.
"""
import math

import numpy as np

F = np.float32
U = 2.0 ** -24                      # one rounding
MAX_RATIO = 51
WEIGHT_SCALE = F(16777216.0)
OPACITY_MAX = F(1.0) - F(2.0 ** -23)
BINOM = np.array([[F(math.comb(n, k)) for k in range(MAX_RATIO)] for n in range(MAX_RATIO)], dtype=np.float32)
RELOCATE, ADD = 0, 1


def f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


class Once:
    """The library calls as float64 functions rounded to float32 once."""

    @staticmethod
    def exp(a):
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            return np.exp(f32(a).astype(np.float64)).astype(np.float32)

    @staticmethod
    def log(a):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.log(f32(a).astype(np.float64)).astype(np.float32)

    @staticmethod
    def pow(a, b):
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.power(f32(a).astype(np.float64), f32(b).astype(np.float64)).astype(np.float32)


ONCE = Once()


def logit(p):
    return math.log(p / (1.0 - p))


def sigmoid(x, lib=ONCE):
    with np.errstate(over="ignore"):
        return F(1.0) / (F(1.0) + lib.exp(-f32(x)))


# ---- plan --------------------------------------------------------------------------------------------------------------------------
def weights(opacity, t_opa, lib=ONCE):
    """int64 [n]: floor(sigmoid 2^24), 0 where !(opacity > t_opa)."""
    x = f32(opacity)
    with np.errstate(invalid="ignore"):
        alive = x > F(t_opa)
        w = np.floor(sigmoid(np.where(alive, x, F(0.0)), lib) * WEIGHT_SCALE).astype(np.int64)
    return np.where(alive, w, 0)


def plan(opacity, t_opa, mode=RELOCATE, lib=ONCE, mutant=None):
    """(cdf int64 [n + 1], dead_offsets int64 [n + 1], dead_idx int32 [n_dead])."""
    x = f32(opacity)
    keep_all = mode == ADD or mutant == "dead_keep_weight"
    w = weights(x, -np.inf if keep_all else t_opa, lib)
    with np.errstate(invalid="ignore"):
        dead = ~(x > F(t_opa))
    cdf = np.concatenate([np.zeros(1, np.int64), np.cumsum(w, dtype=np.int64)])
    dead_offsets = np.concatenate([np.zeros(1, np.int64), np.cumsum(dead, dtype=np.int64)])
    return cdf, dead_offsets, np.nonzero(dead)[0].astype(np.int32)


# ---- draw --------------------------------------------------------------------------------------------------------------------------
def draw(cdf, u):
    """parent int32 [m]: the i with cdf[i] <= t < cdf[i + 1], t = min((int64)(u total), total - 1)."""
    cdf, u = np.asarray(cdf, dtype=np.int64), np.asarray(u, dtype=np.float64)
    total = int(cdf[-1])
    if total <= 0:
        return np.full(len(u), -1, np.int32)
    x = u * float(total)
    with np.errstate(invalid="ignore"):
        t = np.where(x >= float(total), total - 1, np.where(x > 0.0, np.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0), 0.0).astype(np.int64))
    t = np.minimum(t, total - 1)
    return (np.searchsorted(cdf[:-1], t, side="right") - 1).astype(np.int32)


def counts(parent, n):
    """int32 [n]: how often each Gaussian was drawn, by two binary searches in the ascending parent."""
    i = np.arange(n, dtype=np.int64)
    p = np.asarray(parent, dtype=np.int64)
    return (np.searchsorted(p, i + 1, side="left") - np.searchsorted(p, i, side="left")).astype(np.int32)


# ---- update ------------------------------------------------------------------------------------------------------------------------
def ratios(count, mutant=None):
    c = np.asarray(count, dtype=np.int64)
    r = c if mutant == "ratio_no_plus_one" else c + 1
    return np.clip(r, 1, 50 if mutant == "clamp_50" else MAX_RATIO)


def relocate_values(opacity, scaling, ratio, min_opacity, lib=ONCE):
    """(o' logits [m], s' logs [m, 3]) of mcmc_relocate, row by row in its order."""
    x, s, r = f32(opacity), f32(scaling), np.asarray(ratio, dtype=np.int64)
    one = F(1.0)
    with np.errstate(all="ignore"):
        o = sigmoid(x, lib)
        inv_ratio = one / r.astype(np.float32)
        on = one - lib.pow(one - o, inv_ratio)
        denom = np.zeros(len(x), np.float32)
        for i in range(1, int(r.max()) + 1 if len(r) else 1):
            active = r >= i
            p, sign = on.copy(), one
            for k in range(i):
                inv_sqrt = one / np.sqrt(F(k + 1))
                denom = np.where(active, denom + ((BINOM[i - 1, k] * sign) * p) * inv_sqrt, denom)
                p = p * on
                sign = -sign
        coeff = o / denom
        oc = np.where(on < F(min_opacity), F(min_opacity), on)
        oc = np.where(oc > OPACITY_MAX, OPACITY_MAX, oc)
        out_o = lib.log(oc / (one - oc))
        out_s = lib.log(lib.exp(s) * coeff[:, None])
    return out_o, out_s


def update(opacity, scaling, parent, min_opacity, lib=ONCE, mutant=None):
    """(opacity', scaling', count): the rows that were drawn get mcmc_relocate(.., min(count + 1, 51))."""
    o, s = f32(opacity).copy(), f32(scaling).copy()
    c = counts(parent, len(o))
    hit = c > 0
    if hit.any():
        o[hit], s[hit] = relocate_values(o[hit], s[hit], ratios(c[hit], mutant), min_opacity, lib)
    return o, s, c


def move(table, parent, dead_idx):
    out = np.asarray(table).copy()
    out[np.asarray(dead_idx)[:len(parent)]] = out[np.asarray(parent)]
    return out


def zero_rows(table, count):
    out = np.asarray(table).copy()
    out[:len(count)][np.asarray(count) > 0] = 0
    return out


# ---- the two rounds, fused -------------------------------------------------------------------------------------------------------------
def relocate_round(tables, moments, min_opacity, u, lib=ONCE, mutant=None):
    """(tables', moments', parent, dead_idx, count).  tables: dict with opacity [n] and scaling [n, 3] among the [n, ...] tables;
    moments: dict of [n, ...] tables; u: ascending float64, one per dead Gaussian (as many as plan finds)."""
    t_opa = F(logit(min_opacity))
    cdf, dead_offsets, dead_idx = plan(tables["opacity"], t_opa, RELOCATE, lib, mutant)
    t = {k: np.asarray(v).copy() for k, v in tables.items()}
    mom = {k: np.asarray(v).copy() for k, v in moments.items()}
    m = len(dead_idx)
    if m == 0 or cdf[-1] == 0:
        return t, mom, np.zeros(0, np.int32), dead_idx, np.zeros(len(t["opacity"]), np.int32)
    parent = draw(cdf, u[:m])
    t["opacity"], t["scaling"], count = update(t["opacity"], t["scaling"], parent, min_opacity, lib, mutant)
    t = {k: move(v, parent, dead_idx) for k, v in t.items()}
    mom = {k: zero_rows(v, count) for k, v in mom.items()}
    if mutant == "zero_dead_moments":
        for v in mom.values():
            v[dead_idx] = 0
    return t, mom, parent, dead_idx, count


def n_new(n, cap_max):
    return max(0, min(int(cap_max), int(1.05 * n)) - n)


def add_round(tables, moments, min_opacity, u, lib=ONCE, mutant=None):
    """(tables', moments', parent, count): len(u) parents drawn from all Gaussians, updated, their rows appended; moments of the
    appended rows and of the parents zero."""
    t_opa = F(logit(min_opacity))
    cdf, _, _ = plan(tables["opacity"], t_opa, ADD, lib)
    t = {k: np.asarray(v).copy() for k, v in tables.items()}
    n = len(t["opacity"])
    parent = draw(cdf, u)
    parent = parent[parent >= 0]
    t["opacity"], t["scaling"], count = update(t["opacity"], t["scaling"], parent, min_opacity, lib, mutant)
    t = {k: np.concatenate([v, v[parent]]) for k, v in t.items()}
    mom = {k: np.concatenate([zero_rows(v, count), np.zeros((len(parent),) + np.asarray(v).shape[1:], np.asarray(v).dtype)])
           for k, v in moments.items()}
    assert all(len(v) == n + len(parent) for v in t.values())
    return t, mom, parent, count


# ---- the noise -----------------------------------------------------------------------------------------------------------------------
def gate(opacity, lib=ONCE, mutant=None):
    one = F(1.0)
    with np.errstate(over="ignore"):
        o = sigmoid(opacity, lib)
        x = o if mutant == "gate_o" else one - o
        return one / (one + lib.exp(F(-100.0) * (x - F(0.995))))


def noise(means, scaling, rotation, opacity, z, scaler, lib=ONCE, mutant=None):
    """means + R diag(exp(2 s)) R^T (z g scaler) in the order of mcmc_noise."""
    mu, s, q, zz = f32(means), f32(scaling), f32(rotation), f32(z)
    one, two, sc = F(1.0), F(2.0), F(scaler)
    with np.errstate(all="ignore"):
        n2 = ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]
        inv = one / np.sqrt(n2)
        w, x, y, z_ = q[:, 0] * inv, q[:, 1] * inv, q[:, 2] * inv, q[:, 3] * inv
        r00, r01, r02 = one - two * (y * y + z_ * z_), two * (x * y - w * z_), two * (x * z_ + w * y)
        r10, r11, r12 = two * (x * y + w * z_), one - two * (x * x + z_ * z_), two * (y * z_ - w * x)
        r20, r21, r22 = two * (x * z_ - w * y), two * (y * z_ + w * x), one - two * (x * x + y * y)
        g = gate(opacity, lib, mutant)
        v0, v1, v2 = (zz[:, 0] * g) * sc, (zz[:, 1] * g) * sc, (zz[:, 2] * g) * sc
        e = lib.exp(two * s)
        t0 = e[:, 0] * ((r00 * v0 + r10 * v1) + r20 * v2)
        t1 = e[:, 1] * ((r01 * v0 + r11 * v1) + r21 * v2)
        t2 = e[:, 2] * ((r02 * v0 + r12 * v1) + r22 * v2)
        return np.stack([mu[:, 0] + ((r00 * t0 + r01 * t1) + r02 * t2), mu[:, 1] + ((r10 * t0 + r11 * t1) + r12 * t2),
                         mu[:, 2] + ((r20 * t0 + r21 * t1) + r22 * t2)], axis=1)


# ---- gsplat's rule, literally, in float64 -----------------------------------------------------------------------------------------
def literal_parents(opacity, min_opacity, u, alive_only=True):
    """The draws of the rule by inverse CDF over the exact probabilities: among the alive Gaussians (relocate) or all (sample_add),
    proportional to sigmoid(opacity) in float64."""
    o = 1.0 / (1.0 + np.exp(-np.asarray(opacity, dtype=np.float64)))
    o = np.nan_to_num(o, nan=0.0)
    idx = np.nonzero(o > float(F(min_opacity)))[0] if alive_only else np.arange(len(o))
    cum = np.cumsum(o[idx])
    at = np.searchsorted(cum, np.asarray(u, dtype=np.float64) * cum[-1], side="right")
    return idx[np.minimum(at, len(idx) - 1)].astype(np.int32)


def literal_compute_relocation(o, s, ratio):
    """gsplat's compute_relocation on activated float64 opacities [m] and scales [m, 3]: (new opacities, new scales), unclamped."""
    o, s = np.asarray(o, dtype=np.float64), np.asarray(s, dtype=np.float64)
    on = 1.0 - np.power(1.0 - o, 1.0 / np.asarray(ratio, dtype=np.float64))
    denom = np.zeros_like(o)
    for j, r in enumerate(np.asarray(ratio)):
        denom[j] = sum(math.comb(i - 1, k) * (-1.0) ** k / math.sqrt(k + 1) * on[j] ** (k + 1) for i in range(1, int(r) + 1) for k in range(i))
    return on, s * (o / denom)[:, None]


def _literal_update(t, parent, min_opacity):
    """_update of gsplat's relocate / sample_add: the drawn rows' new values, in pre-activation float64."""
    n = len(t["opacity"])
    parent = np.asarray(parent, dtype=np.int64)
    o, s = 1.0 / (1.0 + np.exp(-t["opacity"][parent])), np.exp(t["scaling"][parent])
    ratio = np.clip(np.bincount(parent, minlength=n)[parent] + 1, 1, MAX_RATIO)
    on, sn = literal_compute_relocation(o, s, ratio)
    on = np.clip(on, float(F(min_opacity)), 1.0 - 2.0 ** -23)
    t["opacity"][parent] = np.log(on / (1.0 - on))
    t["scaling"][parent] = np.log(sn)
    return np.bincount(parent, minlength=n)


def literal_relocate(tables, moments, min_opacity, parent):
    """gsplat's relocate with the multinomial's result handed in: dead = sigmoid(opacity) <= min_opacity, the drawn rows updated, every
    dead row a copy of its parent's updated row, the parents' moments zero, the dead rows' moments untouched."""
    t = {k: np.asarray(v, dtype=np.float64).copy() for k, v in tables.items()}
    mom = {k: np.asarray(v).copy() for k, v in moments.items()}
    with np.errstate(invalid="ignore"):
        dead = ~(1.0 / (1.0 + np.exp(-t["opacity"])) > float(F(min_opacity)))
    dead_idx = np.nonzero(dead)[0]
    parent = np.asarray(parent, dtype=np.int64)
    assert len(parent) == len(dead_idx)
    count = _literal_update(t, parent, min_opacity)
    for v in t.values():
        v[dead_idx] = v[parent]
    for v in mom.values():
        v[parent] = 0
    return t, mom, dead_idx, count


def literal_sample_add(tables, moments, min_opacity, parent):
    """gsplat's sample_add with the multinomial's result handed in: the drawn rows updated, then appended; zero moments for both."""
    t = {k: np.asarray(v, dtype=np.float64).copy() for k, v in tables.items()}
    parent = np.asarray(parent, dtype=np.int64)
    count = _literal_update(t, parent, min_opacity)
    t = {k: np.concatenate([v, v[parent]]) for k, v in t.items()}
    mom = {}
    for k, v in moments.items():
        v = np.asarray(v).copy()
        v[parent] = 0
        mom[k] = np.concatenate([v, np.zeros((len(parent),) + v.shape[1:], v.dtype)])
    return t, mom, count


def literal_inject_noise(means, scaling, rotation, opacity, z, scaler):
    """gsplat's inject_noise_to_position in float64: covars = M M^T, M = R S; noise = z g(1 - o) scaler; means + covars @ noise."""
    mu, s, q, zz = (np.asarray(a, dtype=np.float64) for a in (means, scaling, rotation, z))
    o = 1.0 / (1.0 + np.exp(-np.asarray(opacity, dtype=np.float64)))
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z_ = q.T
    R = np.stack([np.stack([1 - 2 * (y * y + z_ * z_), 2 * (x * y - w * z_), 2 * (x * z_ + w * y)], axis=1),
                  np.stack([2 * (x * y + w * z_), 1 - 2 * (x * x + z_ * z_), 2 * (y * z_ - w * x)], axis=1),
                  np.stack([2 * (x * z_ - w * y), 2 * (y * z_ + w * x), 1 - 2 * (x * x + y * y)], axis=1)], axis=1)
    M = R * np.exp(s)[:, None, :]
    cov = np.einsum("bij,bkj->bik", M, M)
    with np.errstate(over="ignore"):
        g = 1.0 / (1.0 + np.exp(-100.0 * ((1.0 - o) - 0.995)))
    v = zz * g[:, None] * float(F(scaler))
    return mu + np.einsum("bij,bj->bi", cov, v)


# ---- how far the float32 fused form may lie from the float64 literal one ---------------------------------------------------------------
# u = 2^-24 is one rounding; everything is first order in u; a library call is held to one unit in the last place (2 u relative),
# glibc's and the device's documented figure for expf, logf and powf alike.  With o the activated opacity, a = 1 - o, r the ratio,
# y = a^(1/r), o' = 1 - y:
#   o     = 1 / (1 + expf(-x)): expf 2 u, the sum 1 u, the quotient 1 u: 4 u relative, at most 4 u absolute.
#   a     = 1 - o: 4 u from o and its own rounding: at most 5 u ABSOLUTE, i.e. 5 u / a relative -- this is the cancellation of the rule
#           itself (gsplat computes 1 - o in float32 too), and it is what an almost opaque parent pays.
#   y     the relative error of a enters divided by r; 1 / r is off by u relative, which moves y by |ln a| u / r relative; powf 2 u.
#   o'    = 1 - y: y's error and one rounding:          B_o' = u (1 + y (2 + (5 / a + |ln a|) / r))               (absolute).
#   D     a term C(i-1, k) (-1)^k o'^(k+1) / sqrt(k+1) carries the coefficient's rounding (1 u), k products of the running power (k u),
#         sqrt, reciprocal and two products (4 u): at most (r + 5) u of |term|; the sum of n = r (r + 1) / 2 terms in a fixed order
#         adds (n - 1) u of T = sum |term|; and o' itself being off by B_o' moves D by at most T1 B_o', T1 = sum |term| (k + 1) / o':
#                                                          B_D = u (n + r + 5) T + T1 B_o'.
#         At ratio 51 and o' = 0.2 the largest term is C(50, 9) 0.2^10 / sqrt(10) = 81 against D of order 1: the alternating sum cancels
#         two digits there, and T / |D| is what B_D charges for it.  For the parents a round meets (o' below 0.1) T / |D| stays below 10.
#   s'    log s' = logf(expf(s) (o / D)): B_D / |D| from D, 4 u from o, 2 u from expf, 2 u from quotient and product, and logf's unit in
#         the last place of the result:                    B_s' = B_D / |D| + u (9 + 2 |log s'|)                   (absolute, on the log).
#   logit o' clamped to [min_opacity, 1 - 2^-23] (a clamp moves nothing apart), 1 - o' (1 u, exact at the upper clamp), the quotient
#         (1 u) and logf:                                  B_logit = B_o' / (o' (1 - o')) + u (3 + 2 |logit|)       (absolute).
def relocation_bounds(opacity, scaling, ratio, min_opacity):
    """(B_logit [m], B_s' [m, 3]) for parents with pre-activation float32 opacity [m], scaling [m, 3] and ratio [m]."""
    x, s = np.asarray(opacity, dtype=np.float64), np.asarray(scaling, dtype=np.float64)
    r = np.asarray(ratio, dtype=np.float64)
    o = 1.0 / (1.0 + np.exp(-x))
    a = 1.0 - o
    y = np.power(a, 1.0 / r)
    on = 1.0 - y
    b_on = U * (1.0 + y * (2.0 + (5.0 / a + np.abs(np.log(a))) / r))
    T, T1, D = np.zeros_like(o), np.zeros_like(o), np.zeros_like(o)
    for j, rj in enumerate(np.asarray(ratio)):
        for i in range(1, int(rj) + 1):
            for k in range(i):
                term = math.comb(i - 1, k) * on[j] ** (k + 1) / math.sqrt(k + 1)
                T[j] += term
                T1[j] += term * (k + 1) / on[j]
                D[j] += term * (-1.0) ** k
    b_d = U * (r * (r + 1.0) / 2.0 + r + 5.0) * T + T1 * b_on
    log_s = s + np.log(o / D)[:, None]
    b_s = (b_d / np.abs(D))[:, None] + U * (9.0 + 2.0 * np.abs(log_s))
    oc = np.clip(on, float(F(min_opacity)), 1.0 - 2.0 ** -23)
    b_logit = b_on / (oc * (1.0 - oc)) + U * (3.0 + 2.0 * np.abs(np.log(oc / (1.0 - oc))))
    return b_logit, b_s


# The noise: g = 1 / (1 + expf(-100 ((1 - o) - 0.995))).  1 - o is off by 5 u absolute (above), the float32 0.995 by u / 2, the
# difference rounds (1 u): 7 u, times 100, and the product rounds (u |arg|, |arg| < 100): the argument is off by 800 u ABSOLUTE, so expf
# of it by 802 u relative, g by at most 804 u, v = (z g) scaler by 806 u.  An entry of R is off by at most 25 u absolute (16 u the common
# scaling of q, 9 u its own roundings: tests/densify_ref.py), exp(2 s) by 2 u, and the two three-term sums with their products by 8 u.
# Every d_i is a sum of nine products R_ij E_j R_kj v_k with |R| <= 1, so with E = the largest exp(2 s) of the row and |v|_1 the float64
# 1-norm of v:  |d_i - d_i^64| <= (806 + 2 . 25 + 2 + 8) u . 3 E |v|_1 = 866 u . 3 E |v|_1, and the sum with the mean adds u (|mean_i| + 3 E |v|_1).
NOISE_ROUNDINGS = 867.0


def noise_bound(means, scaling, opacity, z, scaler):
    """[m, 3] float64: U (NOISE_ROUNDINGS 3 E |v|_1 + |mean_i|) of each row."""
    mu, s, zz = (np.asarray(a, dtype=np.float64) for a in (means, scaling, z))
    o = 1.0 / (1.0 + np.exp(-np.asarray(opacity, dtype=np.float64)))
    with np.errstate(over="ignore"):
        g = 1.0 / (1.0 + np.exp(-100.0 * ((1.0 - o) - 0.995)))
    v1 = np.abs(zz * g[:, None] * float(F(scaler))).sum(axis=1)
    reach = 3.0 * np.exp(2.0 * s).max(axis=1) * v1
    return U * (NOISE_ROUNDINGS * reach[:, None] + np.abs(mu))
