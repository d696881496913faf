"""k-NN label transfer without a GPU: the float64 reference against a literal double loop, the C ABI's argument validation, the
label narrowing and the example loaders of the CLI, and the library's exports."""
import ctypes as C
import pickle
import subprocess

import numpy as np
import pytest
import torch

import gsbp_amd
from gsbp_amd import _lib, transfer
from gsbp_amd._lib import GwbpError

import knn_ref


def test_reference_equals_the_double_loop():
    rng = np.random.default_rng(0)
    for (N, M, D, k) in [(7, 9, 3, 1), (5, 12, 8, 4), (4, 6, 1, 6)]:
        Q, S = rng.standard_normal((N, D)).astype(np.float32), rng.standard_normal((M, D)).astype(np.float32)
        S[M // 2] = S[0]  # a tie: the lower index first
        sc, idx = knn_ref.search(Q, S, k)
        sc2, idx2 = knn_ref.search_loop(Q, S, k)
        assert np.array_equal(idx, idx2) and np.abs(sc - sc2).max() < 1e-12
    dup = np.stack([S[0], S[0]])
    assert knn_ref.search(Q[:1], dup, 2)[1].tolist() == [[0, 1]]


def test_reference_vote_is_bincount_argmax():
    labels = np.array([2, 0, 2, 1, 1, 7, -1])
    idx = np.array([[0, 1, 2], [3, 4, 0], [0, 3, 1], [5, 6, 5], [5, 1, 6]])
    lab, cnt = knn_ref.vote(idx, labels, 3)
    assert lab.tolist() == [2, 1, 0, -1, 0]  # row 2: every label once -> the smallest; row 3: nothing valid
    assert cnt.tolist() == [[1, 0, 2], [0, 2, 1], [1, 1, 1], [0, 0, 0], [1, 0, 0]]


def test_new_symbols_are_exported_and_bound():
    out = subprocess.check_output(["nm", "-D", "--defined-only", gsbp_amd.build()], text=True)
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {"gwbp_knn_search", "gwbp_knn_vote"} <= names
    assert {"gwbp_knn_search", "gwbp_knn_vote"} <= set(_lib.EXPORTS) and callable(gsbp_amd.knn_search)
    assert callable(gsbp_amd.transfer_labels)


def _search(N=4, M=8, D=16, k=2, Q=1 << 12, ldq=None, S=1 << 13, lds=None, idx=1 << 14, score=1 << 15):
    return _lib.lib().gwbp_knn_search(N, M, D, k, Q, D if ldq is None else ldq, S, D if lds is None else lds, idx, score, None)


def _vote(N=4, M=8, k=2, idx=1 << 12, labels=1 << 13, nc=3, out=1 << 14, counts=None, ldc=3):
    return _lib.lib().gwbp_knn_vote(N, M, k, idx, labels, nc, out, counts, ldc, None)


def _err():
    return _lib.lib().gwbp_last_error_string().decode()


def test_abi_argument_validation_needs_no_gpu():
    # (fake, never dereferenced pointers: every case is refused before the first HIP call)
    for kw, word in [(dict(k=0), "k must be"), (dict(k=33, M=64), "k must be"), (dict(k=9), "exceeds"), (dict(D=0), "bad sizes"),
                     (dict(M=0), "bad sizes"), (dict(N=-1), "bad sizes"), (dict(ldq=15), "strides"), (dict(lds=15), "strides"),
                     (dict(Q=None), "null"), (dict(S=None), "null"), (dict(idx=None), "null"), (dict(score=None), "null"),
                     (dict(Q=(1 << 12) + 2), "aligned")]:
        assert _search(**kw) == -1, kw
        assert word in _err(), (kw, _err())
    for kw, word in [(dict(k=0), "k must be"), (dict(k=33), "k must be"), (dict(nc=0), "num_classes"), (dict(M=0), "bad sizes"),
                     (dict(counts=1 << 15, ldc=2), "ldc"), (dict(idx=None), "null"), (dict(labels=None), "null"),
                     (dict(out=None), "null")]:
        assert _vote(**kw) == -1, kw
        assert word in _err(), (kw, _err())


def test_python_api_refuses_host_tensors_and_bad_k():
    with pytest.raises(GwbpError, match="HIP tensor"):
        gsbp_amd.knn_search(torch.zeros(4, 8), torch.zeros(4, 8), 1)
    with pytest.raises(GwbpError, match="HIP tensor"):
        gsbp_amd.transfer_labels(torch.zeros(4, 8), torch.zeros(4, 8), torch.zeros(4), k=1)


def test_label_narrowing():
    lab, nc = transfer.narrow_source_labels(np.array([[0.0], [3.0], [1.0]]))  # the reference's [M, 1] float array
    assert lab.dtype == torch.int32 and lab.tolist() == [0, 3, 1] and nc == 4
    lab, nc = transfer.narrow_source_labels(torch.tensor([0, 5, -2, 2 ** 32 + 1]), 3)
    assert lab.tolist() == [0, -1, -1, -1] and nc == 3  # a wide id does not wrap into range
    lab, nc = transfer.narrow_source_labels(torch.tensor([True, False]))
    assert lab.tolist() == [1, 0] and nc == 2
    with pytest.raises(GwbpError, match="whole numbers"):
        transfer.narrow_source_labels(torch.tensor([0.5, 1.0]))
    with pytest.raises(GwbpError, match="whole numbers"):
        transfer.narrow_source_labels(torch.tensor([float("nan")]))
    with pytest.raises(GwbpError, match=r"\[M\] or \[M, 1\]"):
        transfer.narrow_source_labels(torch.zeros(3, 2))


def test_example_loaders(tmp_path):
    f = np.random.default_rng(1).standard_normal((6, 4)).astype(np.float32)
    lab = np.arange(6, dtype=np.float64).reshape(6, 1)
    torch.save({"features": torch.from_numpy(f), "labels": torch.from_numpy(lab)}, tmp_path / "e.pt")
    np.savez(tmp_path / "e.npz", features=f, labels=lab)
    with open(tmp_path / "features_and_labels.pkl", "wb") as fh:
        pickle.dump({"features": f, "labels": lab}, fh)
    for name in ("e.pt", "e.npz", "features_and_labels.pkl"):
        feats, labels = transfer.load_examples(str(tmp_path / name))
        assert feats.dtype == torch.float32 and np.array_equal(feats.numpy(), f)
        assert transfer.narrow_source_labels(labels)[0].tolist() == list(range(6))
    torch.save({"features": torch.zeros(3, 2)}, tmp_path / "bad.pt")
    with pytest.raises(GwbpError, match="features.*labels"):
        transfer.load_examples(str(tmp_path / "bad.pt"))


def test_synthetic_generator_is_seeded():
    a, b = transfer.synthetic_transfer(n=32, m=16, d=8), transfer.synthetic_transfer(n=32, m=16, d=8)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and a[0].shape == (32, 8) and a[2].shape == (16,)


def test_cli_parser():
    import run_transfer
    a = run_transfer.build_parser().parse_args(["--synthetic", "--out", "x.pt", "--counts", "--k", "7"])
    assert a.synthetic and a.counts and a.k == 7 and a.out == "x.pt"
