"""WMF.similar_items / WMF.similar_users on the device against float64 NumPy on the model's own factors (tests/similar_ref.py),
under the rounded-order rule of tests/test_gpu_serving.py with the derived bounds: B' for the dot product, B_cos for the cosine.
Small trained models: k = 16 with biases, k = 64 without, and a float64 model of the cores = 2 variants, which is served from its
float32 device copies."""
import numpy as np
import pytest

import serving_ref as ref
import similar_ref as sref

pytestmark = pytest.mark.gpu

N_USERS, N_ITEMS = 300, 200
MODELS = {"k16-bias": (16, True, 1), "k64": (64, False, 1), "k16-f64": (16, False, 2)}


@pytest.fixture(scope="module", params=list(MODELS))
def model(request):
    from recmodel_amd import WMF, synth
    dim, bias, cores = MODELS[request.param]
    indptr, indices, counts = synth.make_counts(N_USERS, N_ITEMS, 9, seed=5)
    counts_mat = synth.to_scipy(indptr, indices, counts, (N_USERS, N_ITEMS)).astype(np.float64)
    m = WMF(num_items=N_ITEMS, num_users=N_USERS, dim=dim, gamma=0.1, weighted=True, bias=bias)
    m.train(utility_mat=counts_mat, iterations=2, eval_mat=counts_mat, count_mat=counts_mat, cores=cores)
    assert m.items.dtype == (np.float64 if cores > 1 else np.float32) and not m.items.flags.writeable
    return m


def _reference(model, side, queries, metric):
    """(float64 scores [len(queries), rows], bound) on the float32 values the device holds."""
    M = getattr(model, side).astype(np.float32)
    bias = int(model.bias is True)
    rows = np.arange(len(M))
    d, b = sref.dot_matrix_f64(M, M, queries, rows, bias), sref.dot_bound(M, M, queries, rows, bias)
    if metric == "dot":
        return d, b
    inv = sref.inv_norms_f64(M, bias)
    cos = sref.cosine_f64(d, inv[queries], inv)
    return cos, sref.cos_bound(b, inv[queries], inv, cos)


def _check(got, scores, S, B, queries, exclude_self, topn, what):
    n = S.shape[1]
    assert got.dtype == np.int64 and got.shape == (len(queries), topn), what
    for j, q in enumerate(queries):
        elig = np.setdiff1d(np.arange(n), [q]) if exclude_self else np.arange(n)
        k = min(topn, len(elig))
        it = got[j, :k]
        assert (got[j, k:] == -1).all() and np.isin(it, elig).all() and len(np.unique(it)) == k, (what, j)
        best = ref.stable_topn(S[j, elig], k)
        pos = np.searchsorted(elig, it)
        gap = np.abs(S[j, elig][pos] - S[j, elig][best])
        assert (gap <= np.maximum(B[j, elig][pos], B[j, elig][best])).all(), (what, j)
        if scores is not None:
            assert scores.dtype == np.float32 and (scores[j, k:] == -np.inf).all() and (np.diff(scores[j, :k]) <= 0).all(), (what, j)
            assert (np.abs(scores[j, :k].astype(np.float64) - S[j, it]) <= B[j, it]).all(), (what, j)


@pytest.mark.parametrize("metric", ("cosine", "dot"))
@pytest.mark.parametrize("side", ("items", "users"))
def test_similar_against_float64(model, side, metric):
    call = model.similar_items if side == "items" else model.similar_users
    n = getattr(model, side).shape[0]
    queries = np.array([0, n - 1, 15, 16, 17, 3, 3] + list(range(20, 60, 3)))
    S, B = _reference(model, side, queries, metric)
    for exclude_self in (True, False):
        got, scores = call(queries, 10, metric=metric, exclude_self=exclude_self, return_scores=True)
        _check(got, scores, S, B, queries, exclude_self, 10, (side, metric, exclude_self))
        assert np.array_equal(call(list(queries), 10, metric=metric, exclude_self=exclude_self), got)
        if metric == "cosine" and not exclude_self:                  # a row is its own nearest neighbour, where no other row is as near
            own = np.arange(len(queries)), queries
            rest = np.where(np.arange(n)[None, :] == queries[:, None], -np.inf, S + 2 * B)
            clear = S[own] - 2 * B[own] > rest.max(axis=1)
            assert clear.sum() > len(queries) // 2
            assert (got[clear, 0] == queries[clear]).all() and (np.abs(scores[clear, 0] - 1) <= B[own][clear]).all()
        if exclude_self:
            assert not (got == queries[:, None]).any()
    assert np.array_equal(call(queries, 10, metric=metric), call(queries, 10, metric=metric, exclude_self=True))   # the defaults
    assert metric != "cosine" or np.array_equal(call(queries), call(queries, 10, metric="cosine"))


def test_similar_int_and_negative_ids(model):
    n = N_ITEMS
    many = model.similar_items([5, n - 1, 0, n - 2], 7)
    row = model.similar_items(5, 7)
    assert row.shape == (7,) and row.dtype == np.int64 and np.array_equal(row, many[0])
    assert np.array_equal(model.similar_items(-1, 7), many[1]) and np.array_equal(model.similar_items(np.int64(-n), 7), many[2])
    assert np.array_equal(model.similar_items([-n, -2], 7), many[2:])
    rows, scores = model.similar_users(-3, 4, return_scores=True)
    assert rows.shape == scores.shape == (4,) and scores.dtype == np.float32
    assert np.array_equal(rows, model.similar_users([N_USERS - 3], 4)[0])
    assert model.similar_items([], 3).shape == (0, 3)


def test_similar_in_small_batches(model, monkeypatch):
    from recmodel_amd import wmf_model
    queries = np.arange(N_ITEMS)
    want, want_scores = model.similar_items(queries, 5, return_scores=True)
    monkeypatch.setattr(wmf_model, "RECOMMEND_BATCH_USERS", 48)
    got, scores = model.similar_items(queries, 5, return_scores=True)
    assert np.array_equal(got, want) and np.array_equal(scores.view(np.uint32), want_scores.view(np.uint32))


def test_similar_topn_limits(model):
    from recmodel_amd import wmf_model
    assert wmf_model.RECOMMEND_MAX_TOPN == 128
    queries = np.array([0, 7, N_ITEMS - 1])
    S, B = _reference(model, "items", queries, "cosine")
    got, scores = model.similar_items(queries, 128, return_scores=True)
    _check(got, scores, S, B, queries, True, 128, "topn 128")
    with pytest.raises(ValueError):
        model.similar_items(queries, 129)
    wide = model.similar_users([1], 128)
    assert wide.shape == (1, 128) and (wide >= 0).all() and len(np.unique(wide)) == 128


def test_similar_follows_the_public_arrays(model):
    """The cache rule of _device_factors: the frozen arrays of a trained model are uploaded, and their inverse norms computed,
    once; a writable array is read again on every call, so an in-place edit shows; a freshly assigned array shows too."""
    trained = model.items
    try:
        c0 = int(model.bias is True)
        q = int(np.argmax(np.linalg.norm(trained[:, c0:], axis=1)))
        before = model.similar_items(q, 10)
        j = int(np.setdiff1d(np.arange(N_ITEMS), np.append(before, q))[0])
        norms = model._inv_norms["items"]
        assert np.array_equal(model.similar_items(q, 10), before) and model._inv_norms["items"] is norms    # frozen: by identity
        model.items = trained.copy()                                 # writable, the same values
        assert model.items.flags.writeable and np.array_equal(model.similar_items(q, 10), before)
        model.items[j, c0:] = 3 * model.items[q, c0:]               # in place: j now points where q does
        after, scores = model.similar_items(q, 10, return_scores=True)
        assert after[0] == j and abs(float(scores[0]) - 1) < 1e-5 and np.array_equal(after[1:], before[:9])
        fresh = trained.copy()
        fresh[j] = -fresh[q]                                         # a new array: j now points away from q
        fresh.setflags(write=False)
        model.items = fresh
        away = model.similar_items(q, 10)
        assert j not in away and np.array_equal(away, before) and np.array_equal(model.similar_items(q, 10), away)
        last, last_scores = model.similar_items(j, 1, metric="cosine", exclude_self=False, return_scores=True)
        assert last[0] == j and abs(float(last_scores[0]) - 1) < 1e-5
    finally:
        model.items = trained
    assert np.array_equal(model.similar_items(q, 10), before)
