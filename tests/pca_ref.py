"""TEST SUPPORT: float64 numpy restatement of sklearn.decomposition.PCA's covariance_eigh solver (means, centred covariance, eigh,
sign rule), of its transform and of visualize_pca.py's colours; the case maker; and the error bounds of the PCA tests.

Let u = 2^-24.
  * Covariance entries: E_ab = 2 (N + 2) u sum_g |x_ga - mu_a| |x_gb - mu_b| / (N - 1) -- the worst case of an fp32 sum of N
    products in ANY order ((N + 2) u sum |products|, two roundings for the product's factors), doubled for the fp32 mean.  It does
    not depend on the order, so it holds for any slice scheme.
  * Components (Davis-Kahan): the angle between the j-th float64 component and the computed one is at most 2 ||E||_2 / gap_j, gap_j
    the smaller float64 eigengap next to lambda_j; the error matrix is bounded entrywise by the non-negative E, so its spectral
    norm is at most ||E||_2.
  * Eigenvalues (Weyl): |lambda_j - computed| <= ||E||_2.
  * Transform: |Y - Y64| <= 2 (D + 2) u sum_c |x_c - mu_c| |V_jc|, Y64 in float64 from the SAME fp32 mu and V."""
import numpy as np

U = 2.0 ** -24
ANGLE_CAP = 0.05  # rad: every GPU case's angle bound stays below it (asserted on the reference alone), or the check says little

# make_case's arguments (N, D, planted top eigenvalues, floor eigenvalue, seed, sparse) of the fit cases.  Dense Gaussian rows have
# an angle bound of about 3.3 N u trace / gap: 0.038 at N = 20 000, but above the cap at N = 50 000 for ANY three separated
# components (trace / gap >= 6), so that case plants sparse block components (make_case), whose bound is about 4 N u lambda_1 / gap.
FIT_CASES = [
    (20_000, 64, (16.0, 9.0, 4.0, 1.0), 0.05, 0, None),
    (50_000, 36, (3.0, 2.0, 1.0), 0.002, 1, 0.05),
    (4097, 512, (16.0, 9.0, 4.0, 1.0), 0.05, 2, None),
    (3001, 1028, (16.0, 9.0, 4.0, 1.0), 0.05, 3, None),
]


def make_case(N, D, top=(16.0, 9.0, 4.0, 1.0), floor=0.05, seed=0, sparse=None, offset_sigma=5.0):
    """[N, D] float32 rows with a planted spectrum: eigenvalues `top` (as many as fit into D), then `floor`, plus a mean of
    offset_sigma standard deviations of the largest component in every coordinate (random signs): the top components are well
    separated and the centring matters.  sparse None: Gaussian latents in a random rotation of all D coordinates.  sparse = p:
    every top latent is nonzero in a fraction p of the rows only and points in a random direction inside its own block of D /
    len(top) coordinates, over isotropic noise of variance `floor` (groups of channels that light up on few Gaussians): |x_a||x_b|
    is then small across blocks, which keeps ||E||_2 near 2 N u lambda_1 where dense Gaussian rows give 2 N u 0.8 trace."""
    rng = np.random.default_rng(seed)
    if sparse is None:
        lam = np.full(D, floor)
        lam[:min(D, len(top))] = top[:D]
        R, _ = np.linalg.qr(rng.standard_normal((D, D)))
        X = (rng.standard_normal((N, D)) * np.sqrt(lam)) @ R.T
    else:
        X = rng.standard_normal((N, D)) * np.sqrt(floor)
        width = D // len(top)
        for i, lam_i in enumerate(top):
            r = rng.standard_normal(width)
            z = rng.standard_normal(N) * (rng.random(N) < sparse) * np.sqrt(lam_i / sparse)
            X[:, i * width:(i + 1) * width] += np.outer(z, r / np.linalg.norm(r))
    X += offset_sigma * np.sqrt(top[0]) * rng.choice([-1.0, 1.0], D)
    return X.astype(np.float32)


def mean64(X):
    return np.asarray(X, np.float32).astype(np.float64).mean(axis=0)


def centred64(X):
    X = np.asarray(X, np.float32).astype(np.float64)
    return X - X.mean(axis=0)


def cov64(X):
    Xc = centred64(X)
    return Xc.T @ Xc / (X.shape[0] - 1)


def eig_basis(cov, k):
    """(components [k, D], variances [k], ratios [k], all eigenvalues descending) of a symmetric matrix, sklearn's conventions:
    eigenvalues descending, clipped at 0; each component's first entry of largest magnitude positive."""
    w, v = np.linalg.eigh(cov)
    w, v = np.clip(w[::-1], 0.0, None), v[:, ::-1]
    comps = v[:, :k].T.copy()
    lead = comps[np.arange(k), np.abs(comps).argmax(axis=1)]
    comps *= np.where(lead < 0, -1.0, 1.0)[:, None]
    total = w.sum()
    return comps, w[:k].copy(), (w[:k] / total if total > 0 else np.zeros(k)), w


def fit(X, k=3):
    """(mean [D], components [k, D], explained_variance [k], explained_variance_ratio [k]) in float64."""
    comps, var, ratio, _ = eig_basis(cov64(X), k)
    return mean64(X), comps, var, ratio


def transform64(X, mean, comps):
    return (np.asarray(X, np.float32).astype(np.float64) - np.asarray(mean, np.float64)) @ np.asarray(comps, np.float64).T


def colors64(Y):
    lo, hi = Y.min(), Y.max()
    return (Y - lo) / (hi - lo), lo, hi


def cov_bound(X):
    """E [D, D]: the entrywise bound on |computed covariance - cov64(X)|."""
    A = np.abs(centred64(X))
    N = X.shape[0]
    return 2.0 * (N + 2) * U * (A.T @ A) / (N - 1)


def angle_bounds(X, k=3, E=None):
    """(theta [k], ||E||_2): the Davis-Kahan angle bound of each of the top k components."""
    E = cov_bound(X) if E is None else E
    norm = np.linalg.norm(E, 2)
    w = np.linalg.eigvalsh(cov64(X))[::-1]
    theta = np.empty(k)
    for j in range(k):
        gaps = [w[j - 1] - w[j]] if j > 0 else []
        if j + 1 < len(w):
            gaps.append(w[j] - w[j + 1])
        theta[j] = 2.0 * norm / min(gaps)
    return theta, norm


def angle(v, w):
    """The angle in [0, pi / 2] between the lines of two vectors (atan2 of the rejection and the projection: exact near 0)."""
    v, w = np.asarray(v, np.float64), np.asarray(w, np.float64)
    v, w = v / np.linalg.norm(v), w / np.linalg.norm(w)
    c = abs(v @ w)
    return float(np.arctan2(np.linalg.norm(w - (v @ w) * v), c))


def transform_bound(X, mean, comps):
    X = np.asarray(X, np.float32).astype(np.float64)
    return 2.0 * (X.shape[1] + 2) * U * (np.abs(X - np.asarray(mean, np.float64)) @ np.abs(np.asarray(comps, np.float64)).T)


def shifted(X, sigmas=100.0):
    """The rows plus a constant vector of `sigmas` standard deviations of each column (away from zero: with the sign of the column's
    mean), rounded to fp32: the same spread on a far larger mean (what an uncentred Gram cannot take)."""
    X = np.asarray(X, np.float32)
    X64 = X.astype(np.float64)
    shift = sigmas * X64.std(axis=0) * np.where(X64.mean(axis=0) < 0, -1.0, 1.0)
    return (X + shift.astype(np.float32)).astype(np.float32)


def cov_bound_with_mean(X):
    """E' [D, D] >= the error of an fp32 centred covariance whatever the spread: cov_bound's doubling covers the fp32 mean only while
    a column's spread is far above one ulp of its mean.  With the computed mean mu (1 + e), |e| <= u, the exact Gram moves by N d d^T
    (d_a = e mu_a; the cross terms vanish because sum_g (x_g - mu) = 0), and the centred values grow by at most |d|:
        E'_ab = [(N + 2) u (1 + u)^2 sum_g (|x_ga - mu_a| + u |mu_a|)(|x_gb - mu_b| + u |mu_b|) + N u^2 |mu_a mu_b|] / (N - 1).
    Used where a case has columns that nearly coincide (N = 2 rows at a mean of 20: 63 entries of the EXACT fp32 evaluation exceed
    cov_bound there, by the N d d^T term)."""
    N = X.shape[0]
    m = U * np.abs(mean64(X))
    A = np.abs(centred64(X)) + m
    return ((N + 2) * U * (1.0 + U) ** 2 * (A.T @ A) + N * np.outer(m, m)) / (N - 1)
