"""numpy float64 reference of the field comparison (gsbp_amd.fidelity), written from its definition, and the seeded scene of its tests.

    r(p, :)  = sum over the oracle's contributing (Gaussian, pixel) pairs of w F[g, :]          (oracle.blend_pairs, float64 sums)
    dot, rr, mm, l1, l2 = sum_c r m, r r, m m, |r - m|, (r - m)^2          cosine = dot / sqrt(rr mm), NaN where rr mm == 0
    a pixel whose map row holds a non-finite value: NaN in every plane, counted in n_bad; valid: finite planes and rr mm > 0

scale(p) of a plane is the sum of the absolute values of its terms: the size against which a rounding or a moved weight shows.
A pixel is SENSITIVE when one of its planes moves by more than TOL * scale under a 2-ulp change of exp() (the method of
tests/test_sensitivity.py): its pairs sit on the alpha >= 1/255 or T <= 1e-4 cuts, where a kernel may decide either way.
"""
import functools

import numpy as np

from gsbp_amd import synthetic as syn
from oracle import oracle as orc

TOL = 1e-4  # tests/test_gpu_parity.py: fp32 sums against the oracle
W, H = 70, 45  # 5 x 3 tiles, the last column 6 pixels wide, the last row 13 high
N = 3000
SEED = 21
N_VIEWS = 4
CFG = syn.Config("FID", N, N_VIEWS, W, H, 32, 0.08, False)
NAMES = ("dot", "rr", "mm", "l1", "l2")


@functools.lru_cache(maxsize=None)
def scene():
    """Host tensors: (means, quats, scales, opac), viewmats [4, 4, 4], K [3, 3]."""
    gauss = tuple(t.contiguous() for t in syn.activate(syn.make_scene(CFG, seed=SEED)))
    return gauss, syn.make_cameras(CFG), syn.intrinsics(CFG)


def feature_map(view, dim):
    """float32 [H, W, dim] on the host (synthetic.make_feature_map: unit rows)."""
    return syn.make_feature_map(CFG, view, dim=dim)


def _pairs(view):
    (means, quats, scales, opac), vms, K = scene()
    proj = orc.project(means.numpy(), quats.numpy(), scales.numpy(), vms[view].numpy(), K.numpy(), W, H)
    bins = orc.bin_sort(proj, W, H)
    return orc.blend_pairs(proj, bins, opac.numpy(), W, H, want_alphas=True)


@functools.lru_cache(maxsize=None)
def pairs(view):
    """(gid, pix, w, alphas [H, W]) of the oracle as it is.  Shared: do not write into them."""
    return _pairs(view)


def render64(pr, field):
    """float64 [H W, D]: the render of `field` [N, D] from the pairs pr."""
    gid, pix, w, _ = pr
    out = np.zeros((H * W, field.shape[1]), np.float64)
    np.add.at(out, pix, w.astype(np.float64)[:, None] * field.astype(np.float64)[gid])
    return out


def planes_of(r, m):
    """({name: float64 [H, W]} with cosine, valid, bad; {name: scale [H, W]}) of a render r [H W, D] (any float type) and a map
    m [H, W, D]."""
    r = np.asarray(r, np.float64).reshape(H, W, -1)
    m = np.asarray(m, np.float64)
    bad = ~np.isfinite(m).all(axis=-1)
    mz = np.where(bad[..., None], 0.0, m)
    df = r - mz
    terms = dict(dot=r * mz, rr=r * r, mm=mz * mz, l1=np.abs(df), l2=df * df)
    p = {k: t.sum(axis=-1) for k, t in terms.items()}
    scale = {k: np.abs(t).sum(axis=-1) for k, t in terms.items()}
    den = p["rr"] * p["mm"]
    with np.errstate(invalid="ignore", divide="ignore"):
        p["cosine"] = np.where(den > 0, p["dot"] / np.sqrt(np.where(den > 0, den, 1.0)), np.nan)
    for k in p:
        p[k] = np.where(bad, np.nan, p[k])
    p["bad"] = bad
    p["valid"] = ~bad & (den > 0) & np.isfinite(np.stack([p[k] for k in NAMES])).all(axis=0)
    return p, scale


def table_of(p, dim):
    v = p["valid"]
    return np.array([p["cosine"][v].sum(), p["l1"][v].sum(), p["l2"][v].sum(), p["mm"][v].sum(), v.sum(), p["bad"].sum(), H * W, dim],
                    np.float64)


def reference(view, field, m):
    """planes_of on the oracle's render of `field` for `view`."""
    return planes_of(render64(pairs(view), field), m)


def sensitive(view, field, m):
    """bool [H, W]: pixels where a 2-ulp exp() moves a plane by more than TOL * scale."""
    base, scale = reference(view, field, m)
    out = np.zeros((H, W), bool)
    try:
        for ulp in (2, -2):
            orc.set_tunables(exp_ulp=ulp)
            moved, _ = planes_of(render64(_pairs(view), field), m)
            for k in NAMES:
                out |= np.abs(moved[k] - base[k]) > TOL * np.maximum(scale[k], 1e-30)
    finally:
        orc.set_tunables()
    return out


def block_of_view2():
    """The 20 x 20 block of view 2's map that test 7 replaces by random vectors: (y0, y1, x0, x1)."""
    return 12, 32, 25, 45


def corrupt(m, seed=5):
    """A copy of the float32 map m [H, W, D] whose block is unit random vectors."""
    y0, y1, x0, x1 = block_of_view2()
    out = np.array(m, np.float32, copy=True)
    noise = np.random.default_rng(seed).standard_normal((y1 - y0, x1 - x0, m.shape[2])).astype(np.float32)
    out[y0:y1, x0:x1] = noise / np.linalg.norm(noise, axis=-1, keepdims=True)
    return out


@functools.lru_cache(maxsize=None)
def consistent_maps(dim, seed=77):
    """float32 [H, W, dim] maps of the four views that DO describe one 3-D scene: the renders of a seeded unit-row truth field,
    each pixel normalised (a pixel nothing covers stays zero).  synthetic.make_feature_map draws every pixel of every view
    independently: a Gaussian that k pixels see gets the mean of k independent unit vectors, whose cosine with any one of them is
    about 1 / sqrt(k), so NO field lifted from such maps agrees with them (measured with this reference: mean cosine 0.09, and
    cosine >= 0.5 fails at 98.9 % of the covered pixels); an agreement test needs maps a field can agree with.  Shared: do not
    write into them."""
    truth = np.random.default_rng(seed).standard_normal((N, dim)).astype(np.float32)
    truth /= np.linalg.norm(truth, axis=1, keepdims=True)
    out = []
    for v in range(N_VIEWS):
        r = render64(pairs(v), truth).reshape(H, W, dim)
        n = np.linalg.norm(r, axis=-1, keepdims=True)
        m = np.where(n > 0, r / np.where(n > 0, n, 1.0), 0.0).astype(np.float32)
        m.setflags(write=False)
        out.append(m)
    return tuple(out)
