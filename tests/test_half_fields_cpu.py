"""fp16 / bf16 finished fields without a GPU: the *_typed entry points exist in every layer, refuse bad arguments before any HIP call
(fake pointers, never dereferenced), and finalize_reference rounds once, to nearest even, as the integer reference of
tests/half_fields_ref.py does."""
import os
import re

import numpy as np
import pytest
import torch

import gsbp_amd
from gsbp_amd import _lib
from gsbp_amd.backproject import finalize_reference

import half_fields_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F16, BF16 = 0, 1, 2
TYPED = ("gwbp_finalize_typed", "gwbp_prompt_scores_typed", "gwbp_neighbor_similarity_typed", "gwbp_neighbor_mean_typed",
         "gwbp_neighbor_blend_typed", "gwbp_knn_search_typed", "gwbp_kmeans_assign_typed", "gwbp_cluster_sums_typed",
         "gwbp_column_means_typed", "gwbp_centered_gram_typed", "gwbp_pca_project_typed")


def test_typed_entry_points_exist_in_every_layer():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gwbp.h")).read(), flags=re.S)
    declared = set(re.findall(r"GWBP_API int (gwbp_[a-z0-9_]+)\(", header))
    capi = open(os.path.join(_lib.CSRC, "capi.hip")).read()
    gsbp_amd.build()
    for name in TYPED:
        assert name in declared, name
        assert re.search(r"^int %s\(" % name, capi, flags=re.M), name
        assert name in _lib.EXPORTS and name in _lib.FIELD_ARGTYPES, name
        fn = getattr(_lib.lib(), name)  # resolves in the built library, with its argument types set
        assert fn is not None and list(fn.argtypes) == _lib.FIELD_ARGTYPES[name] and _lib.FIELD_ARGTYPES[name].count(_lib._I32) >= 2
    assert _lib.MAP_F32 == F32 and _lib.MAP_F16 == F16 and _lib.MAP_BF16 == BF16


# ---- argument validation ---------------------------------------------------------------------------------------------------------------
P = [1 << s for s in range(12, 24)]  # fake, 4-KiB aligned, never dereferenced
WS = 1 << 30


def _err():
    return _lib.lib().gwbp_last_error_string().decode()


# every call below: (X = the field pointer, t = its type code, ld = its row stride) first, then what the untyped function's own
# checks look at
def _scores(X=P[0], t=F16, ld=16, N=40, D=16, Pn=3, n_pos=2, prompts=P[1], thr=None, mask=P[2], scores=P[3]):
    return _lib.lib().gwbp_prompt_scores_typed(N, D, Pn, n_pos, X, t, ld, prompts, 1, thr, mask, scores, None)


def _sim(X=P[0], t=F16, ld=16, n=40, D=16, k=4, idx=P[1], sim=P[2], live=P[3]):
    return _lib.lib().gwbp_neighbor_similarity_typed(n, D, k, idx, X, t, ld, sim, live, None)


def _mean(X=P[0], t=F16, ld=16, n=40, m=40, D=16, k=4, idx=P[1], out=P[2], ldo=16):
    return _lib.lib().gwbp_neighbor_mean_typed(n, m, D, k, idx, X, t, ld, out, ldo, None)


def _blend(X=P[0], t=F16, ld=16, q=40, m=40, D=16, k=4, idx=P[1], w=P[2], out=P[3], ldo=16, wsum=P[4]):
    return _lib.lib().gwbp_neighbor_blend_typed(q, m, D, k, idx, w, X, t, ld, out, ldo, wsum, None)


def _knn(X=P[0], t=F16, ld=16, N=40, M=8, D=16, k=4, S=P[1], lds=16, idx=P[2], score=P[3]):
    return _lib.lib().gwbp_knn_search_typed(N, M, D, k, X, t, ld, S, lds, idx, score, None)


def _assign(X=P[0], t=F16, ld=16, N=40, K=7, D=16, C=P[1], ldc=16, b=P[2], label=P[3], best=P[4]):
    return _lib.lib().gwbp_kmeans_assign_typed(N, K, D, X, t, ld, C, ldc, b, label, best, None)


def _sums(X=P[0], t=F16, ld=16, N=40, D=16, K=7, w=None, order=P[1], start=P[2], sums=P[3], wsum=P[4], ws=P[5], ws_bytes=WS):
    return _lib.lib().gwbp_cluster_sums_typed(N, D, K, X, t, ld, w, order, start, sums, wsum, ws, ws_bytes, None)


def _means(X=P[0], t=F16, ld=16, N=40, D=16, mean=P[1], ws=P[2], ws_bytes=WS):
    return _lib.lib().gwbp_column_means_typed(N, D, X, t, ld, mean, ws, ws_bytes, None)


def _gram(X=P[0], t=F16, ld=16, N=40, D=16, mean=P[1], gram=P[2], ws=P[3], ws_bytes=WS):
    return _lib.lib().gwbp_centered_gram_typed(N, D, X, t, ld, mean, gram, ws, ws_bytes, None)


def _project(X=P[0], t=F16, ld=16, N=40, D=16, k=3, mean=P[1], comps=P[2], Y=P[3], mm=P[4]):
    return _lib.lib().gwbp_pca_project_typed(N, D, k, X, t, ld, mean, comps, Y, mm, None)


def _finalize(out=P[0], t=F16, N=40, D=16, F=P[1], d=P[2]):
    return _lib.lib().gwbp_finalize_typed(N, D, F, d, out, t, None)


# the untyped functions' own invalid cases, through the typed entry point with a half field
OWN = {
    _scores: [dict(N=-1), dict(Pn=0), dict(Pn=33), dict(n_pos=0), dict(n_pos=4), dict(D=0), dict(D=2049, ld=4096), dict(X=None),
              dict(prompts=None), dict(prompts=P[1] + 2), dict(mask=None, scores=None), dict(scores=P[3] + 2),
              dict(Pn=2, n_pos=2)],
    _sim: [dict(n=0), dict(k=0), dict(k=65), dict(idx=None), dict(sim=None), dict(sim=P[2] + 2), dict(D=0), dict(D=2049, ld=4096),
           dict(X=None), dict(live=None), dict(live=P[3] + 1), dict(sim=P[0]), dict(live=P[2])],
    _mean: [dict(n=-1), dict(m=0), dict(D=0), dict(k=0), dict(k=33), dict(ldo=15), dict(X=None), dict(idx=None), dict(out=None),
            dict(out=P[2] + 2), dict(out=P[0])],
    _blend: [dict(q=-1), dict(m=0), dict(k=0), dict(k=33), dict(idx=None), dict(w=P[2] + 1), dict(D=0), dict(ldo=15), dict(X=None),
             dict(out=None), dict(wsum=P[4] + 2), dict(out=P[0]), dict(wsum=P[3])],
    _knn: [dict(N=-1), dict(M=0), dict(D=0), dict(k=0), dict(k=33), dict(k=9), dict(lds=15), dict(S=None), dict(X=None),
           dict(idx=None), dict(S=P[1] + 2)],
    _assign: [dict(N=-1), dict(K=0), dict(K=(1 << 20) + 1), dict(D=0), dict(X=None), dict(ldc=15), dict(C=None), dict(label=None),
              dict(C=P[1] + 2), dict(b=P[2] + 2)],
    _sums: [dict(N=-1), dict(K=0), dict(D=0), dict(X=None), dict(start=None), dict(order=None), dict(sums=None), dict(ws=None),
            dict(w=P[6] + 2), dict(order=P[1] + 4), dict(sums=P[3] + 4)],
    _means: [dict(N=1), dict(D=0), dict(D=2049, ld=4096), dict(X=None), dict(ws=None), dict(ws=P[2] + 4), dict(mean=None)],
    _gram: [dict(N=1), dict(D=0), dict(X=None), dict(ws=None), dict(mean=None), dict(gram=None), dict(gram=P[2] + 4)],
    _project: [dict(N=0), dict(D=0), dict(D=2049, ld=4096), dict(k=0), dict(k=17), dict(X=None), dict(mean=None), dict(comps=None),
               dict(Y=None), dict(mm=None)],
    _finalize: [dict(N=-1), dict(D=0), dict(F=None), dict(d=None), dict(out=None)],
}


@pytest.mark.parametrize("call", list(OWN), ids=lambda f: f.__name__.strip("_"))
def test_typed_entry_points_refuse_bad_arguments_before_any_hip_call(call):
    gsbp_amd.build()
    # an unknown type code, checked before anything else: even with every other argument bad
    for t in (-1, 3, 7):
        assert call(t=t) == -1 and "type" in _err(), (t, _err())
    bad_everything = dict(out=None, N=-5) if call is _finalize else dict(X=None, ld=-1)
    assert call(t=9, **bad_everything) == -1 and "unknown" in _err(), _err()
    # a half element at an odd address; an fp32 element at a 2-B aligned one (the untyped function's rule)
    field = "out" if call is _finalize else "X"
    for t in (F16, BF16):
        assert call(t=t, **{field: P[0] + 1}) == -1 and "aligned" in _err(), (t, _err())
    assert call(t=F32, **{field: P[0] + 2}) == -1 and "aligned" in _err(), _err()
    if call is not _finalize:  # a row stride, in elements, below D
        for t in (F32, F16, BF16):
            assert call(t=t, ld=15) == -1 and "stride" in _err(), (t, _err())
    for t in (F32, F16, BF16):
        for kw in OWN[call]:
            assert call(t=t, **kw) == -1, (t, kw)
            assert _err(), kw


def test_finalize_typed_refuses_a_half_out_that_aliases_F():
    gsbp_amd.build()
    for t in (F16, BF16):
        assert _finalize(out=P[1], t=t) == -1 and "alias" in _err(), _err()
    with pytest.raises(ValueError):
        finalize_reference(torch.ones(2, 4), torch.ones(2), torch.float64)


def test_workspace_shortfall_is_reported_as_such():
    gsbp_amd.build()
    assert _means(ws_bytes=8) == -2 and _gram(ws_bytes=8) == -2 and _sums(ws_bytes=8) == -2


# ---- the two roundings -----------------------------------------------------------------------------------------------------------------
def _accumulators(width: int, ties):
    g = torch.Generator().manual_seed(1234)
    n = 96
    F = torch.randn(n, width, generator=g)
    d = torch.rand(n, generator=g) + 0.5
    F[:, 1::3] *= 1e-6  # fp16 subnormals beside entries of order 1 ...
    F[:, 2::5] *= 1e-9  # ... and results that underflow to zero
    d[0] = 0.0          # x / 1e-12: large, then normalised
    F[1] = 0.0          # 0 / 0 = NaN -> 0
    F[2], d[2] = 0.0, 0.0
    for i, m in enumerate(ties):  # rows the finalise returns unchanged (d = 1, norm exactly 1): exact ties reach the rounding
        F[3 + 2 * i] = torch.from_numpy(ref.tie_row(m, width))
        F[4 + 2 * i] = -F[3 + 2 * i]
        d[3 + 2 * i] = d[4 + 2 * i] = 1.0
    return F, d


@pytest.mark.parametrize("dtype,bits,ties", [(torch.float16, ref.f32_to_f16_bits, ref.F16_TIES),
                                             (torch.bfloat16, ref.f32_to_bf16_bits, ref.BF16_TIES)], ids=["fp16", "bf16"])
def test_finalize_reference_rounds_once_to_nearest_even(dtype, bits, ties):
    F, d = _accumulators(23, ties)
    full = finalize_reference(F.clone(), d.clone())
    assert full.dtype == torch.float32 and torch.equal(full, finalize_reference(F.clone(), d.clone(), torch.float32))
    assert not bool(torch.isnan(full).any()) and bool((full[1] == 0).all()) and bool((full[2] == 0).all())
    half = finalize_reference(F.clone(), d.clone(), dtype)
    assert half.dtype == dtype and half.shape == F.shape
    got = half.contiguous().view(torch.int16).numpy().view(np.uint16)
    want = bits(full.numpy())
    assert np.array_equal(got, want)
    # the cases the reference is there for do occur
    for i, m in enumerate(ties):
        assert np.array_equal(full[3 + 2 * i].numpy(), ref.tie_row(m, 23))  # the tie arrived exactly
        lo, hi = (m // 2 * 2, m // 2 * 2 + 2) if dtype == torch.float16 else (m // 16 * 16, m // 16 * 16 + 16)
        step = 2 if dtype == torch.float16 else 16
        even = lo if (lo // step) % 2 == 0 else hi
        assert float(half[3 + 2 * i, 0]) == even * 2.0 ** -12 and float(half[4 + 2 * i, 0]) == -even * 2.0 ** -12
    if dtype == torch.float16:
        mag = full.abs()
        assert bool(((mag > 0) & (mag < 2.0 ** -25)).any()) and bool(((mag > 2.0 ** -24) & (mag < 2.0 ** -14)).any())
        sub = half[(mag > 2.0 ** -24) & (mag < 2.0 ** -15)].float().abs()
        assert bool((sub > 0).any()) and bool((sub < 2.0 ** -14).all())  # subnormal results are kept, not flushed
        assert bool((half[(mag > 0) & (mag < 2.0 ** -26)] == 0).all())    # and what lies below half the smallest one is zero
