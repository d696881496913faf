"""float64 numpy reference of the prompt queries (gsbp_amd.segment), its rounding bound and the seeded cases of the tests.

    s[g, j] = x_g . t_j / max(|x_g|, 1e-12)      (normalize)      s[g, j] = x_g . t_j      (otherwise)
    mask[g] = max_{j < n_pos} s[g, j] > max_{j >= n_pos} s[g, j]   (and s[g, 0] > thr;  n_pos == P: the threshold test alone)

Rounding bound, u = 2^-24: a score computed as one fp32 fused-multiply-add chain over D channels, a chain for the sum of squares, a
correctly rounded sqrt and a correctly rounded divide differs from the float64 one by at most
    B[g, j] = (D + 4) u sum_c |x_gc| |t_jc| / |x_g|          (without the denominator when not normalising).
A row is DECIDED when its float64 margin |max_pos - max_neg| exceeds 2 max_j B[g, j] -- both maxima may move by max_j B -- and, with
a threshold, |s[g, 0] - thr| exceeds B[g, 0] as well.  On a decided row every computation within the bound gives the float64 mask.
"""
import numpy as np

U = 2.0 ** -24

# (N, D, P, n_pos)
CASES = [(20000, 512, 4, 1), (50000, 16, 3, 1), (4097, 1028, 32, 5), (3001, 30, 2, 1)]


def make_case(n, d, p, n_pos, seed=0, centres=8, noise=0.7):
    """A mixture of `centres` cluster centres plus noise x sigma noise, row scales 0.1 .. 10 (log-uniform); the prompts are noisy
    normalised centres (prompt j belongs to centre j mod centres).  float32 arrays (X [n, d], T [p, d])."""
    rng = np.random.default_rng(1000 * seed + 7 * n + d + p)
    c = rng.standard_normal((centres, d))
    x = c[rng.integers(0, centres, n)] + noise * rng.standard_normal((n, d))
    x *= 10.0 ** rng.uniform(-1.0, 1.0, (n, 1))
    t = c[np.arange(p) % centres] + 0.3 * rng.standard_normal((p, d))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    return x.astype(np.float32), t.astype(np.float32)


def scores(x, t, normalize=True):
    x, t = np.asarray(x, np.float64), np.asarray(t, np.float64)
    s = x @ t.T
    if normalize:
        s = s / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)
    return s


def bound(x, t, normalize=True):
    """B [N, P]."""
    x, t = np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(t, np.float64))
    b = (x.shape[1] + 4) * U * (x @ t.T)
    if normalize:
        b = b / np.maximum(np.sqrt((x * x).sum(axis=1, keepdims=True)), 1e-300)
    return b


def mask_of(s, n_pos, thr=None):
    p = s.shape[-1]
    m = s[..., :n_pos].max(axis=-1) > s[..., n_pos:].max(axis=-1) if n_pos < p else np.ones(s.shape[:-1], bool)
    if thr is not None:
        m = m & (s[..., 0] > thr)
    return m


def decided(s, b, n_pos, thr=None):
    """bool [N]: rows whose mask cannot be changed by errors within b."""
    p = s.shape[-1]
    ok = np.ones(s.shape[:-1], bool)
    if n_pos < p:
        ok &= np.abs(s[..., :n_pos].max(axis=-1) - s[..., n_pos:].max(axis=-1)) > 2.0 * b.max(axis=-1)
    if thr is not None:
        ok &= np.abs(s[..., 0] - thr) > b[..., 0]
    return ok


def threshold_of(s):
    """A threshold for prompt 0 that lies between its scores' two modes (rows of its own cluster, the others): the midpoint of the
    5th and the 95th percentile -- where few rows are, unlike the median."""
    lo, hi = np.percentile(s[:, 0], [5.0, 95.0])
    return float(np.float32(0.5 * (lo + hi)))


def two_blob_scene(n_per=300, d=32, seed=3):
    """Two separated blobs of Gaussians in front of a camera at the origin looking down +z, with a field that is one direction per
    blob plus noise: the click tests' "objects".  Returns a dict of float32 numpy arrays and the two blob centres' pixels."""
    rng = np.random.default_rng(seed)
    W, H = 96, 64
    centres = np.array([[-0.45, 0.0, 3.0], [0.45, 0.0, 3.0]])
    means = np.concatenate([c + 0.12 * rng.standard_normal((n_per, 3)) for c in centres])
    quats = rng.standard_normal((2 * n_per, 4))
    scales = np.exp(np.log(0.05) + 0.2 * rng.standard_normal((2 * n_per, 3)))
    opac = rng.uniform(0.5, 0.95, 2 * n_per)
    dirs = rng.standard_normal((2, d))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    feats = np.repeat(dirs, n_per, axis=0) + 0.05 * rng.standard_normal((2 * n_per, d))
    K = np.array([[80.0, 0, W / 2], [0, 80.0, H / 2], [0, 0, 1]])
    vm = np.eye(4)
    pix = [(int(K[0, 0] * c[0] / c[2] + K[0, 2]), int(K[1, 1] * c[1] / c[2] + K[1, 2])) for c in centres]
    f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    return dict(means=f32(means), quats=f32(quats), scales=f32(scales), opac=f32(opac), feats=f32(feats), K=f32(K), viewmat=f32(vm),
                width=W, height=H, pixels=pix)
