"""WMF.candidates, WMF.candidates_for and the device path of WMF.recommend beyond 128 (wmf_recommend_topn_wide) against the routes
they replace or restate: the loop over rank(), recommend() up to 128 bit for bit, predict() for the scores, and candidates() on a
model whose users are fold_in(count_rows).  EXACT-class factors (tests/serving_ref.py): integer scores and real ties, so every
comparison is for equality."""
import numpy as np
import pytest
import scipy.sparse as sp

import serving_ref as ref

pytestmark = pytest.mark.gpu

N_USERS, N_ITEMS, F = 40, 3000, 5


@pytest.fixture(scope="module")
def model():
    from recmodel_amd import WMF
    m = WMF(num_items=N_ITEMS, num_users=N_USERS, dim=F - 1, gamma=0.1, weighted=True, bias=True)
    m.users, m.items = ref.exact_factors(N_USERS, F, 10 * F + 1), ref.exact_factors(N_ITEMS, F, 10 * F + 4)
    return m


@pytest.fixture(scope="module")
def train():
    t = sp.random(N_USERS, N_ITEMS, density=0.1, format="lil", random_state=3, dtype=np.float32)
    t[7, :] = 1.0                                                   # user 7 has seen everything, user 8 all but two items
    t[8, 2:] = 1.0
    t[8, :2] = 0.0
    return sp.csr_matrix(t)


@pytest.fixture(scope="module")
def by_rank(model, train):
    """The loop over rank() at the largest n, once: a shorter list is its prefix (the order is total)."""
    users = list(range(N_USERS)) + [3, 3]
    out = np.full((len(users), 1000), -1, dtype=np.int64)
    for j, u in enumerate(users):
        cand = np.setdiff1d(np.arange(N_ITEMS), train[u].indices)
        best = model.rank(cand, int(u), 1000) if len(cand) else cand
        out[j, :len(best)] = best
    out.setflags(write=False)
    return users, out


def _same(a, b):
    return all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b)) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))


@pytest.mark.parametrize("n", (10, 129, 1000))
def test_candidates_against_rank_and_predict(model, train, by_rank, n):
    users, want = by_rank
    items, scores = model.candidates(users, n, exclude=train, return_scores=True)
    assert items.dtype == np.int64 and items.shape == (len(users), n) and scores.dtype == np.float32
    assert np.array_equal(items, want[:, :n])
    assert np.array_equal(model.candidates(users, n, exclude=train), items)
    assert (items[7] == -1).all() and (scores[7] == -np.inf).all()
    assert set(items[8, :2]) == {0, 1} and (items[8, 2:] == -1).all()
    valid = items >= 0
    assert (scores[~valid] == -np.inf).all()
    uu = np.repeat(np.asarray(users), valid.sum(axis=1))
    assert np.array_equal(scores[valid], model.predict(uu, items[valid]).astype(np.float32))
    row = model.candidates(5, n, exclude=train)
    assert row.shape == (n,) and np.array_equal(row, items[5])


@pytest.mark.parametrize("n", (1, 10, 128))
def test_candidates_up_to_128_is_recommend_bit_for_bit(model, train, n):
    users = list(range(N_USERS)) + [3, 3]
    mask = np.random.default_rng(11).random(N_ITEMS) < 0.2
    for kw in ({}, dict(allow=mask), dict(allow=np.flatnonzero(mask))):
        assert _same(model.candidates(users, n, exclude=train, return_scores=True, **kw),
                     model.recommend(users, n, exclude=train, return_scores=True, **kw)), (n, list(kw))


def test_recommend_beyond_128_takes_the_device_path(model, train, by_rank, monkeypatch):
    from recmodel_amd import WMF, wmf_model
    users, want = by_rank
    got = model.recommend(users, 200, exclude=train, return_scores=True)
    assert _same(got, model.candidates(users, 200, exclude=train, return_scores=True))
    assert np.array_equal(got[0], want[:, :200])
    over = wmf_model.CANDIDATES_MAX + 1                               # beyond the wide kernels: still the loop over rank()
    assert over > N_ITEMS
    host = model.recommend([0, 8], over, exclude=train)
    assert host.shape == (2, over) and np.array_equal(host[0, :1000], want[0]) and (host[1, 2:] == -1).all()
    calls = []

    def no_rank(self, *a, **k):
        calls.append(a)
        raise AssertionError("recommend() went through rank()")
    monkeypatch.setattr(WMF, "rank", no_rank)
    assert _same(model.recommend(users, 200, exclude=train, return_scores=True), got) and not calls
    assert np.array_equal(model.recommend(users, wmf_model.CANDIDATES_MAX, exclude=train)[:, :200], got[0]) and not calls
    with pytest.raises(AssertionError, match="went through rank"):
        model.recommend([0], over, exclude=train)
    assert len(calls) == 1


def _counts(B):
    counts = sp.random(B, N_ITEMS, density=0.02, format="lil", random_state=4, dtype=np.float32)
    counts[1, :] = 0.0                                                # an empty history
    counts = sp.csr_matrix(counts)
    counts.eliminate_zeros()
    counts.data[:] = np.ceil(counts.data * 5)
    return counts


def test_candidates_for_is_candidates_on_the_folded_in_rows(model):
    from recmodel_amd import WMF
    B = 9
    counts = _counts(B)
    assert counts[1].nnz == 0
    folded = WMF(num_items=N_ITEMS, num_users=B, dim=F - 1, gamma=0.1, weighted=True, bias=True)
    folded.users, folded.items = model.fold_in(counts), model.items
    mask = np.random.default_rng(12).random(N_ITEMS) < 0.3
    shelves = np.stack([mask, ~mask])
    allow_idx = np.arange(B) % 3 - 1
    for kw in ({}, dict(allow=mask), dict(allow=np.flatnonzero(mask)), dict(allow=shelves, allow_idx=allow_idx)):
        got = model.candidates_for(counts, 500, return_scores=True, **kw)
        assert got[0].dtype == np.int64 and got[0].shape == (B, 500) and got[1].dtype == np.float32
        assert _same(got, folded.candidates(np.arange(B), 500, exclude=counts, return_scores=True, **kw)), list(kw)
        assert np.array_equal(model.candidates_for(counts, 500, **kw), got[0])
        for b in range(B):
            seen = set(counts[b].indices)
            assert not seen & set(got[0][b]) and len(set(got[0][b])) == 500
    free = model.candidates_for(counts, 500, exclude_history=False, return_scores=True)
    assert _same(free, folded.candidates(np.arange(B), 500, return_scores=True))
    small = model.candidates_for(counts, 10, return_scores=True)
    assert _same(small, model.recommend_for(counts, 10, return_scores=True))
    assert (model.candidates_for(counts, 500, allow=[]) == -1).all()
    assert model.candidates_for(sp.csr_matrix((0, N_ITEMS)), 300).shape == (0, 300)


def test_a_failed_row_has_no_candidates():
    """tests/test_gpu_foldin_model.py's indefinite row: unit vectors as items, alpha = -3 on a linear transform."""
    from recmodel_amd import WMF
    n = 400
    m = WMF(num_items=n, num_users=3, dim=8, gamma=0.1, weighted=True)
    m.items = np.zeros((n, 8), dtype=np.float32)
    m.items[np.arange(n), np.arange(n) % 8] = 1.0
    m.users = np.zeros((3, 8), dtype=np.float32)
    rows = sp.csr_matrix((np.array([400.0, 0.1]), np.array([3, 5]), np.array([0, 1, 1, 2])), shape=(3, n))
    X = m.fold_in(rows, alpha=-3, pre_process_count="linear")
    assert np.isnan(X[0]).all() and (X[1] == 0).all() and np.isfinite(X[2]).all()
    items, scores = m.candidates_for(rows, 200, return_scores=True, alpha=-3, pre_process_count="linear")
    assert (items[0] == -1).all() and np.isneginf(scores[0]).all()
    assert np.array_equal(items[1], np.arange(200)) and (scores[1] == 0).all()
    assert (items[2] >= 0).all() and 5 not in items[2]


def test_small_batches_and_a_small_workspace_give_the_same_output(model, train, monkeypatch):
    from recmodel_amd import _lib, wmf_model
    users = list(range(N_USERS)) + [3, 3, 11]
    counts = _counts(7)
    want = model.candidates(users, 300, exclude=train, return_scores=True)
    want_for = model.candidates_for(counts, 300, return_scores=True)
    shelves = np.random.default_rng(13).random((3, N_ITEMS)) < 0.5
    allow_idx = np.arange(len(users)) % 4 - 1
    want_rows = model.candidates(users, 300, exclude=train, return_scores=True, allow=shelves, allow_idx=allow_idx)
    monkeypatch.setattr(wmf_model, "RECOMMEND_BATCH_USERS", 3)
    assert len(users) % 3 != 0
    assert _same(model.candidates(users, 300, exclude=train, return_scores=True), want)
    assert _same(model.candidates_for(counts, 300, return_scores=True), want_for)
    assert _same(model.candidates(users, 300, exclude=train, return_scores=True, allow=shelves, allow_idx=allow_idx), want_rows)
    monkeypatch.setattr(wmf_model, "RECOMMEND_BATCH_USERS", 4096)
    ws = _lib.load().wmf_recommend_wide_workspace_bytes
    one = int(ws(1, 300, 0))
    assert int(ws(2, 300, 0)) > one
    for bound in (one, one - 1, 5 * one):                            # one row fills a call (it is never fewer), then a few rows
        monkeypatch.setattr(wmf_model, "CANDIDATES_WS_BYTES", bound)
        assert _same(model.candidates(users, 300, exclude=train, return_scores=True), want), bound
        assert _same(model.recommend(users, 300, exclude=train, return_scores=True), want), bound
        assert _same(model.candidates(users, 300, exclude=train, return_scores=True, allow=shelves, allow_idx=allow_idx), want_rows), bound
    assert _same(model.candidates_for(counts, 300, return_scores=True), want_for)
