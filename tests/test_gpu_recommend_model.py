"""WMF.recommend and utils.test_coverage on the device, against the formulation they replace: rank() of the unseen items,
user by user (RecModel/utils.py:3-17).  The model's factors are EXACT-class arrays (tests/serving_ref.py): integer scores, real
ties, so every comparison is for equality."""
import numpy as np
import pytest
import scipy.sparse as sp

import serving_ref as ref

pytestmark = pytest.mark.gpu

N_USERS, N_ITEMS, F = 40, 300, 5


@pytest.fixture(scope="module")
def model():
    from recmodel_amd import WMF
    m = WMF(num_items=N_ITEMS, num_users=N_USERS, dim=F - 1, gamma=0.1, weighted=True, bias=True)
    m.users, m.items = ref.exact_factors(N_USERS, F, 10 * F + 1), ref.exact_factors(N_ITEMS, F, 10 * F + 2)
    return m


@pytest.fixture(scope="module")
def train():
    t = sp.random(N_USERS, N_ITEMS, density=0.15, format="lil", random_state=3, dtype=np.float32)
    t[7, :] = 1.0                                                   # user 7 has seen everything, user 8 all but two items
    t[8, 2:] = 1.0
    t[8, :2] = 0.0
    t = sp.csr_matrix(t)
    assert t[7].nnz == N_ITEMS and t[8].nnz == N_ITEMS - 2
    t.data[::5] = 0.0                                               # stored zeros count as seen
    assert t.nnz > (t.data != 0).sum()
    return t


def _by_rank(model, train, users, topn):
    everything = np.arange(N_ITEMS)
    out = np.full((len(users), topn), -1, dtype=np.int64)
    for j, u in enumerate(users):
        unseen = np.delete(everything, train[u].indices) if train is not None else everything
        best = model.rank(unseen, int(u), topn) if len(unseen) else unseen
        out[j, :len(best)] = best
    return out


@pytest.mark.parametrize("topn", (1, 10, 128))
def test_recommend_is_rank_of_the_unseen_items(model, train, topn):
    users = list(range(N_USERS)) + [3, 3]
    got = model.recommend(users, topn, exclude=train)
    assert got.dtype == np.int64 and got.shape == (len(users), topn)
    assert np.array_equal(got, _by_rank(model, train, users, topn))
    assert (got[7] == -1).all() and (got[8, :2] >= 0).all() and (got[8, 2:] == -1).all() if topn > 2 else True
    assert np.array_equal(model.recommend(users, topn), _by_rank(model, None, users, topn))          # nothing excluded


def test_recommend_in_small_batches(model, train, monkeypatch):
    from recmodel_amd import wmf_model
    want = model.recommend(np.arange(N_USERS), 10, exclude=train)
    monkeypatch.setattr(wmf_model, "RECOMMEND_BATCH_USERS", 16)
    got, scores = model.recommend(np.arange(N_USERS), 10, exclude=train, return_scores=True)
    assert np.array_equal(got, want) and np.array_equal(got, _by_rank(model, train, range(N_USERS), 10))
    assert scores.dtype == np.float32 and scores.shape == got.shape


def test_recommend_beyond_the_fused_maximum_falls_back_to_rank(model, train):
    users = [0, 7, 8, 21]
    got, scores = model.recommend(users, 200, exclude=train, return_scores=True)
    assert np.array_equal(got, _by_rank(model, train, users, 200)) and got.shape == (4, 200)
    fused = model.recommend(users, 128, exclude=train)
    assert np.array_equal(got[:, :128], fused)
    valid = got >= 0
    assert (scores[~valid] == -np.inf).all() and (np.diff(scores[0][valid[0]]) <= 0).all()


def test_recommend_int_and_negative_users(model, train):
    row = model.recommend(5, 10, exclude=train)
    assert row.shape == (10,) and np.array_equal(row, _by_rank(model, train, [5], 10)[0])
    assert np.array_equal(model.recommend(-1, 10, exclude=train), _by_rank(model, train, [N_USERS - 1], 10)[0])
    got = model.recommend([-N_USERS, -2, 4], 3, exclude=train)
    assert np.array_equal(got, _by_rank(model, train, [0, N_USERS - 2, 4], 3))
    items, scores = model.recommend(np.int64(6), 4, return_scores=True)
    assert items.shape == scores.shape == (4,)


def test_recommend_scores_match_predict(model, train):
    users = np.arange(N_USERS)
    items, scores = model.recommend(users, 10, exclude=train, return_scores=True)
    valid = items >= 0
    assert scores.dtype == np.float32 and (scores[~valid] == -np.inf).all() and 0 < (~valid).sum() < valid.sum()
    want = model.predict(np.repeat(users, valid.sum(axis=1)), items[valid])
    assert np.array_equal(scores[valid], want.astype(np.float32))


def test_coverage_on_the_device_is_the_loop_over_rank(model, train):
    from recmodel_amd import utils
    topn = 4
    got = utils.test_coverage(model, train, topn)
    want = np.zeros(N_ITEMS, dtype=np.int32)
    for u in range(N_USERS):
        unseen = np.delete(np.arange(N_ITEMS, dtype=np.int32), train.indices[train.indptr[u]:train.indptr[u + 1]])
        if len(unseen):
            want[model.rank(users=u, items=unseen, topn=topn)[:topn]] += 1
    assert got.dtype == np.int32 and np.array_equal(got, want)
    eligible = N_ITEMS - np.diff(train.indptr)
    assert got.sum() == np.minimum(eligible, topn).sum() and want[N_USERS:].sum() > 0
    full = sp.csr_matrix((N_USERS, N_ITEMS), dtype=np.float32)
    assert utils.test_coverage(model, full, topn).sum() == N_USERS * topn
