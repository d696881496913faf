"""The PCA's reference (tests/pca_ref.py) against sklearn, the host logic of gsbp_amd.pca on CPU tensors, and -- on the reference
alone -- the cap that keeps the GPU test's angle bounds meaningful."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gsbp_amd
from gsbp_amd import pca

import pca_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_equals_sklearn():
    """sklearn gets the float64 copy of the fp32 rows.  (On the fp32 rows themselves it works in fp32 and forms the UNCENTRED
    covariance: with this case's mean of 20 against a spread of 0.7 per coordinate its variances are off by 1.3e-4 relative -- the
    cancellation the product's centred Gram avoids -- while signed cosines still agree to 1e-4.)"""
    decomposition = pytest.importorskip("sklearn.decomposition")
    X = pca_ref.make_case(*pca_ref.FIT_CASES[0])
    sk32 = decomposition.PCA(3).fit(X)
    assert sk32._fit_svd_solver == "covariance_eigh"
    assert all(float(sk32.components_[j] @ pca_ref.fit(X, 3)[1][j]) > 1.0 - 1e-4 for j in range(3))
    sk = decomposition.PCA(3).fit(X.astype(np.float64))
    assert sk._fit_svd_solver == "covariance_eigh"
    mean, comps, var, ratio = pca_ref.fit(X, 3)
    for j in range(3):
        assert float(sk.components_[j] @ comps[j]) > 1.0 - 1e-4  # the cosine WITH its sign
    np.testing.assert_allclose(sk.explained_variance_, var, rtol=1e-4)
    np.testing.assert_allclose(sk.explained_variance_ratio_, ratio, rtol=1e-4)
    np.testing.assert_allclose(sk.mean_, mean, rtol=1e-4)
    Y = pca_ref.transform64(X, mean, comps)
    np.testing.assert_allclose(sk.transform(X.astype(np.float64)), Y, rtol=1e-4, atol=1e-4 * np.abs(Y).max())


def test_sign_rule_and_descending_order():
    cov = torch.tensor([[2.0, -1.0, 0.0], [-1.0, 2.0, 0.0], [0.0, 0.0, 5.0]], dtype=torch.float64)
    comps, var, ratio = pca._eig_basis(cov, 3)
    assert torch.allclose(var, torch.tensor([5.0, 3.0, 1.0], dtype=torch.float64))
    assert torch.allclose(ratio, var / 9.0)
    r = 0.5 ** 0.5
    # eigenvalue 3 has (1, -1) / sqrt 2: two entries of equal magnitude, the FIRST is made positive; eigenvalue 1 has (1, 1) / sqrt 2
    want = torch.tensor([[0.0, 0.0, 1.0], [r, -r, 0.0], [r, r, 0.0]], dtype=torch.float64)
    assert torch.allclose(comps, want, atol=1e-12)
    ref_comps, ref_var, ref_ratio, _ = pca_ref.eig_basis(cov.numpy(), 3)
    assert np.allclose(ref_comps, want.numpy(), atol=1e-12) and np.allclose(ref_var, var.numpy())
    # a component whose largest entry is negative is flipped as a whole
    v = torch.tensor([-0.8, 0.6], dtype=torch.float64)
    comps, var, _ = pca._eig_basis(4.0 * torch.outer(v, v), 1)
    assert torch.allclose(comps[0], -v, atol=1e-12) and abs(float(var[0]) - 4.0) < 1e-12
    # no spread: finite components, variance and ratio 0; a small negative eigenvalue is clipped
    comps, var, ratio = pca._eig_basis(torch.zeros(4, 4, dtype=torch.float64), 3)
    assert bool(torch.isfinite(comps).all()) and float(var.abs().max()) == 0.0 and float(ratio.abs().max()) == 0.0
    with pytest.raises(gsbp_amd.GwbpError, match="NaN"):
        pca._eig_basis(torch.full((2, 2), float("nan"), dtype=torch.float64), 1)


def test_argument_errors():
    with pytest.raises(gsbp_amd.GwbpError, match="HIP tensor"):
        gsbp_amd.fit_pca(torch.randn(10, 4))
    with pytest.raises(gsbp_amd.GwbpError, match="HIP tensor"):
        gsbp_amd.pca_colors(torch.randn(10, 4))
    with pytest.raises(gsbp_amd.GwbpError, match=r"n_components must be in \[1, 16\]"):
        gsbp_amd.fit_pca(torch.randn(10, 40), 17)
    with pytest.raises(gsbp_amd.GwbpError, match="n_components must be"):
        gsbp_amd.fit_pca(torch.randn(10, 40), 0)
    with pytest.raises(gsbp_amd.GwbpError, match="exceeds D"):
        gsbp_amd.fit_pca(torch.randn(10, 2), 3)
    with pytest.raises(gsbp_amd.GwbpError, match="at least 2 rows"):
        gsbp_amd.fit_pca(torch.randn(1, 4))
    with pytest.raises(gsbp_amd.GwbpError, match=r"D must be in \[1, 2048\]"):
        gsbp_amd.fit_pca(torch.randn(4, 2049))
    with pytest.raises(gsbp_amd.GwbpError, match=r"\[N, D\]"):
        gsbp_amd.fit_pca(torch.randn(4, 3, 2))
    with pytest.raises(ValueError, match="mode"):
        next(gsbp_amd.render_pca(*[None] * 9, mode="gif"))


def test_c_abi_rejects_bad_arguments_before_any_hip_call():
    import ctypes as C
    lib = gsbp_amd.lib()
    n = C.c_size_t(0)
    assert lib.gwbp_pca_workspace_size(1_000_000, 512, C.byref(n)) == 0
    # 10 tiles of the upper triangle -> 51 slices of [512, 512] fp32 partials; the figure does not grow with N
    assert n.value == 51 * 512 * 512 * 4
    m = C.c_size_t(0)
    assert lib.gwbp_pca_workspace_size(4_000_000, 512, C.byref(m)) == 0 and m.value == n.value
    for d in (1, 100, 128, 129, 640, 1024, 2048):
        assert lib.gwbp_pca_workspace_size(5_000_000, d, C.byref(m)) == 0 and m.value <= 64 << 20
    assert lib.gwbp_pca_workspace_size(1, 4, C.byref(n)) == -1
    assert lib.gwbp_pca_workspace_size(10, 2049, C.byref(n)) == -1
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.gwbp_column_means(1, 4, p, 4, p, p, 512, None) == -1                       # N < 2
    assert lib.gwbp_column_means(8, 4, p, 3, p, p, 512, None) == -1                       # stride below D
    assert lib.gwbp_column_means(8, 4, p, 4, p, p, 8, None) == -2                         # workspace too small
    assert b"workspace" in lib.gwbp_last_error_string()
    assert lib.gwbp_centered_gram(8, 4, p, 4, p, None, p, 1 << 20, None) == -1            # null gram_out
    assert lib.gwbp_centered_gram(8, 4, C.c_void_p(p.value + 2), 4, p, p, p, 1 << 20, None) == -1  # misaligned X
    assert lib.gwbp_pca_project(8, 4, 17, p, 4, p, p, p, p, None) == -1                   # k > 16
    assert lib.gwbp_pca_project(8, 4, 0, p, 4, p, p, p, p, None) == -1
    assert lib.gwbp_pca_project(8, 4, 3, p, 4, p, p, p, None, None) == -1                 # null partials
    assert lib.gwbp_pca_colors(-1, p, p, p, None) == -1
    assert lib.gwbp_pca_colors(4, p, None, p, None) == -1


def test_basis_round_trips_through_its_state_dict():
    b = pca.PCABasis(torch.arange(4.0), torch.eye(3, 4), torch.tensor([3.0, 2.0, 1.0], dtype=torch.float64),
                     torch.tensor([0.5, 0.3, 0.2], dtype=torch.float64), 7)
    c = pca.PCABasis.from_state_dict(b.state_dict())
    assert torch.equal(c.mean, b.mean) and torch.equal(c.components, b.components) and c.n_samples == 7
    assert torch.equal(c.explained_variance, b.explained_variance)


def test_frame_conversion_on_cpu_tensors():
    lo, hi = torch.tensor(-1.0), torch.tensor(3.0)
    v = torch.tensor([[[-2.0, -1.0, 0.0], [1.0, 3.0, 5.0]]])
    assert pca._to_uint8("renderings", v, lo, hi).tolist() == [[[0, 0, 63], [127, 255, 255]]]  # truncation, saturation
    assert pca._to_uint8("renderings", v, lo, lo).dtype == torch.uint8                          # no spread: no division by 0
    c = torch.tensor([[[-0.5, 0.0, 0.999], [0.5, 1.0, 1.5]]])
    assert pca._to_uint8("gaussians", c, lo, hi).tolist() == [[[0, 0, 254], [127, 255, 255]]]


def test_run_pca_help():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_pca.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "--mode" in r.stdout and "--synthetic" in r.stdout and "--scale" in r.stdout


@pytest.mark.parametrize("case", range(len(pca_ref.FIT_CASES)))
def test_angle_bounds_of_the_gpu_cases_stay_under_the_cap(case):
    """On the reference alone: the Davis-Kahan bound of each of the top 3 components of every case of test_gpu_pca.py's fit test
    is at most 0.05 rad, for the case itself and for its 100-sigma shifted copy (the centring test)."""
    X = pca_ref.make_case(*pca_ref.FIT_CASES[case])
    theta, norm = pca_ref.angle_bounds(X)
    print(pca_ref.FIT_CASES[case][:2], "angle bounds", theta, "||E||_2", norm)
    assert (theta <= pca_ref.ANGLE_CAP).all()
    if case == 0:
        theta, _ = pca_ref.angle_bounds(pca_ref.shifted(X))
        assert (theta <= pca_ref.ANGLE_CAP).all()
