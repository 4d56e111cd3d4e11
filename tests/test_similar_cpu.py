"""tests/similar_ref.py -- the host reference of wmf_row_inv_norms / wmf_similar_topn -- against a brute-force float64 cosine and
dot product on Gaussian factors, its zero-row and self rules, the size of NumPy's own float32 error against the derived bound, and
the argument checks of WMF.similar_items / similar_users, which come before any GPU use.  No GPU."""
import numpy as np
import pytest

import serving_ref as ref
import similar_ref as sref

N_ROWS, N_QUERIES, TOPN = 300, 40, 10
WIDTHS = (4, 5, 16, 64, 65, 129, 260)


def _brute(C, bias, q, metric, self_out, topn):
    """Row by row with np.dot and np.linalg.norm, ordered by a Python sort on (-score, id)."""
    scored = []
    for j in range(len(C)):
        if self_out and j == q:
            continue
        d = float(np.dot(C[q, bias:].astype(np.float64), C[j, bias:].astype(np.float64)))
        if metric == "cosine":
            nq, nj = np.linalg.norm(C[q, bias:].astype(np.float64)), np.linalg.norm(C[j, bias:].astype(np.float64))
            d = d / (nq * nj) if nq > 0 and nj > 0 else 0.0
        scored.append((-d, j))
    scored.sort()
    return np.array([j for _, j in scored[:topn]]), np.array([-s for s, _ in scored[:topn]])


@pytest.mark.parametrize("bias", (0, 1))
@pytest.mark.parametrize("f", WIDTHS)
def test_reference_against_brute_force(f, bias):
    C = ref.rounded_factors(N_ROWS, f, 7 * f + bias)
    C[5] = 0                                                        # a zero row: cosine 0 with everything
    queries = np.random.default_rng(f).choice(N_ROWS, N_QUERIES, replace=False)
    queries[0] = 5
    rows = np.arange(N_ROWS)
    d = sref.dot_matrix_f64(C, C, queries, rows, bias)
    inv = sref.inv_norms_f64(C, bias)
    assert inv[5] == 0 and (inv[np.arange(N_ROWS) != 5] > 0).all()
    assert np.allclose(sref.inv_norms_ref(C, bias), inv, rtol=2.0 ** -23, atol=0)
    cos = sref.cosine_f64(d, inv[queries], inv)
    for scores, metric in ((d, "dot"), (cos, "cosine")):
        for b, q in enumerate(queries):
            for self_out in (True, False):
                got = sref.similar_ref(scores[b], q if self_out else None, [], TOPN)
                want, want_scores = _brute(C, bias, int(q), metric, self_out, TOPN)
                assert len(got) == TOPN and (not self_out or q not in got)
                # the same rows, up to the order of scores that agree to float64 rounding
                assert np.allclose(scores[b, got], want_scores, rtol=0, atol=1e-12 * max(1.0, np.abs(want_scores).max())), (f, bias, metric, q)
                if (np.abs(np.diff(want_scores)) > 1e-9).all():
                    assert np.array_equal(got, want), (f, bias, metric, q)
    own = cos[np.arange(N_QUERIES), queries]
    assert np.abs(own[queries != 5] - 1).max() < 1e-12 and (own[queries == 5] == 0).all()    # a row's cosine with itself


def test_inverse_norm_rules():
    M = np.zeros((8, 6), dtype=np.float32)
    M[1, 0] = 3.0                                                    # only the bias column
    M[2] = [0, 3, 4, 0, 0, 0]
    M[3] = np.float32(2.0) ** -149 * np.arange(1, 7)                 # small subnormals: the inverse overflows float32
    M[4] = np.float32(2.0) ** 60 * np.array([0, 3, 4, 0, 0, 0], dtype=np.float32)
    M[5] = np.float32(2.0) ** -60 * np.array([0, 3, 4, 0, 0, 0], dtype=np.float32)
    M[6] = [1, 0, 0, 0, 0, 0]
    M[7] = [5, 0, 0, 0, 0, -2]
    r1, r0 = sref.inv_norms_ref(M, 1), sref.inv_norms_ref(M, 0)
    assert r1.dtype == np.float32 and np.array_equal(r1, np.array([0, 0, 0.2, 0, 0.2 * 2.0 ** -60, 0.2 * 2.0 ** 60, 0, 0.5], dtype=np.float32))
    assert r0[0] == 0 and r0[1] == np.float32(1 / 3) and r0[2] == np.float32(0.2) and r0[3] == 0 and r0[6] == 1
    assert r0[7] == np.float32(1 / np.sqrt(29.0))


def test_scale_and_self_rules():
    d = np.array([[3, 0, -3, 6, 12]], dtype=np.int64)
    sq, si = np.array([0.5], dtype=np.float32), np.array([1, 1, 1, 0.5, 0.25], dtype=np.float32)
    s = sref.scale_f32(d, sq, si)
    assert s.dtype == np.float32 and s.tolist() == [[1.5, 0, -1.5, 1.5, 1.5]]
    # the order of the two multiplications is part of the contract: one rounding each
    a, b, c = np.float32(1 + 2.0 ** -23), np.float32(1 + 2.0 ** -12), np.float32(1 - 2.0 ** -12)
    assert sref.scale_f32([[a]], [b], [c])[0, 0] == np.float32(np.float32(a * b) * c)
    # ties after scaling go to the lower row; the row itself and the excluded rows are left out, duplicates and all
    assert sref.similar_ref(s[0], None, [], 3).tolist() == [0, 3, 4]
    assert sref.similar_ref(s[0], 0, [], 3).tolist() == [3, 4, 1]
    assert sref.similar_ref(s[0], 3, [4, 4, 0], 5).tolist() == [1, 2]
    assert sref.similar_ref(s[0], 3, [3], 2).tolist() == [0, 4]
    assert sref.similar_ref(np.array([1.0]), 0, [], 4).tolist() == []
    # -0.0 = +0.0
    assert sref.similar_ref(np.array([0.0, -0.0, 0.0], dtype=np.float32), None, [], 3).tolist() == [0, 1, 2]


@pytest.mark.parametrize("bias", (0, 1))
@pytest.mark.parametrize("f", (4, 16, 64, 129, 260))
def test_float32_arithmetic_stays_inside_the_bound(f, bias):
    """B_cos is derived, not measured: NumPy's own float32 evaluation of the header's formula has to sit well inside it."""
    C = ref.rounded_factors(N_ROWS, f, 10 * f + 2)
    rows = np.arange(N_ROWS)
    q = rows[:N_QUERIES]
    d32 = C[q][:, bias:] @ C[:, bias:].T                               # float32 sums, in whatever order BLAS takes
    inv32, inv64 = sref.inv_norms_ref(C, bias), sref.inv_norms_f64(C, bias)
    got = (d32 * inv32[q][:, None]) * inv32[None, :]
    cos = sref.cosine_f64(sref.dot_matrix_f64(C, C, q, rows, bias), inv64[q], inv64)
    bound = sref.cos_bound(sref.dot_bound(C, C, q, rows, bias), inv64[q], inv64, cos)
    ratio = float((np.abs(got.astype(np.float64) - cos) / bound).max())
    print(f"f={f} bias={bias}: float32 NumPy error / B_cos = {ratio:.3f}")
    assert ratio < 0.5


# ----------------------------------------------------------------------------------------- the Python surface, before any GPU use
def _model(bias=False, users=True):
    from recmodel_amd import WMF
    m = WMF(num_items=30, num_users=20, dim=4, gamma=0.1, weighted=True, bias=bias)
    if users:
        m.users = np.random.default_rng(0).random((20, m.items.shape[1])).astype(np.float32)
    return m


def _no_gpu(monkeypatch):
    from recmodel_amd import _lib

    def touched():
        raise AssertionError("the GPU was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "require_gpu", touched)


@pytest.mark.parametrize("bias", (False, True))
def test_argument_checks_come_before_the_gpu(monkeypatch, bias):
    from recmodel_amd import wmf_model
    _no_gpu(monkeypatch)
    m = _model(bias)
    for call, n in ((m.similar_items, 30), (m.similar_users, 20)):
        with pytest.raises(ValueError, match="metric"):
            call([0], metric="euclid")
        with pytest.raises(ValueError, match="topn"):
            call([0], topn=0)
        with pytest.raises(ValueError, match="topn"):
            call(0, topn=wmf_model.RECOMMEND_MAX_TOPN + 1)
        for bad in (n, -n - 1, [0, n], [-n - 1]):
            with pytest.raises(IndexError):
                call(bad)
        with pytest.raises(AssertionError, match="GPU was touched"):   # good arguments do reach the device
            call([0, -1, n - 1, -n], topn=wmf_model.RECOMMEND_MAX_TOPN)


def test_similar_users_before_training(monkeypatch):
    _no_gpu(monkeypatch)
    m = _model(users=False)
    assert m.users is None
    with pytest.raises((AttributeError, ValueError)):
        m.similar_users([0])


def test_similar_items_before_training(monkeypatch):
    """No user factors yet: the device copies are of both matrices, so similar_items says so too, before the GPU is touched."""
    _no_gpu(monkeypatch)
    m = _model(users=False)
    with pytest.raises(AttributeError, match="user factors"):
        m.similar_items([0])
    with pytest.raises(AttributeError, match="user factors"):
        m.similar_items(3, metric="dot")


def test_docstring_says_there_is_no_fallback():
    from recmodel_amd import WMF
    assert "RECOMMEND_MAX_TOPN" in WMF.similar_items.__doc__ and "ValueError" in WMF.similar_items.__doc__
