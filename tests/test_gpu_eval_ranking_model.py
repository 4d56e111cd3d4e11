"""WMF.rank_positions and RecModel.eval_ranking on the device, against the host reference (tests/rankpos_ref.py) and against the
formulation they replace: rank() of the unseen items, user by user, and a look-up of the held-out items in the returned order.
The model's factors are EXACT-class arrays (tests/serving_ref.py): integer scores, real ties, so every comparison of ranks is for
equality."""
import numpy as np
import pytest
import scipy.sparse as sp

import rankpos_ref as pref
import serving_ref as ref

pytestmark = pytest.mark.gpu

N_USERS, N_ITEMS, F = 40, 300, 5
TOPN = np.array([1, 10, 50, 128, 300])


@pytest.fixture(scope="module")
def model():
    from recmodel_amd import WMF
    m = WMF(num_items=N_ITEMS, num_users=N_USERS, dim=F - 1, gamma=0.1, weighted=True, bias=True)
    m.users, m.items = ref.exact_factors(N_USERS, F, 10 * F + 1), ref.exact_factors(N_ITEMS, F, 10 * F + 2)
    return m


@pytest.fixture(scope="module")
def scores():
    M = ref.score_matrix_int(ref.exact_factors(N_USERS, F, 10 * F + 1), ref.exact_factors(N_ITEMS, F, 10 * F + 2), np.arange(N_USERS),
                             np.arange(N_ITEMS), True)
    M.setflags(write=False)
    return M


@pytest.fixture(scope="module")
def train():
    t = sp.random(N_USERS, N_ITEMS, density=0.15, format="lil", random_state=3, dtype=np.float32)
    t[7, :] = 1.0                                                   # user 7 has seen everything, user 8 all but two items
    t[8, 2:] = 1.0
    t[8, :2] = 0.0
    t = sp.csr_matrix(t)
    t.data[::5] = 0.0                                               # stored zeros count as seen
    return t


@pytest.fixture(scope="module")
def held_out(train):
    from recmodel_amd import wmf_model
    t = sp.random(N_USERS, N_ITEMS, density=0.02, format="lil", random_state=4, dtype=np.float32)
    t[5, :] = 0.0                                                   # user 5 has no held-out items
    t[6, ::3] = 1.0                                                 # user 6 has 100: the host splits the row
    t[7, 10] = 1.0                                                  # a user who has seen everything still has held-out items
    t[8, :4] = 1.0                                                  # two of them unseen, two seen
    t[9, train[9].indices[:3]] = 2.0                                # seen targets
    t = sp.csr_matrix(t)
    t.eliminate_zeros()
    t.data[::7] = 0.0                                               # stored zeros are targets
    assert t[5].nnz == 0 and t[6].nnz > 2 * wmf_model.RANKPOS_MAX_TARGETS and t[7].nnz > 0
    return t


def _want(scores, held_out, train, users):
    """(indptr, indices, ranks) of the reference, for the canonical rows of `users`."""
    rows, idx = [], []
    for u in users:
        t = np.unique(held_out[u].indices)
        idx.append(t)
        rows.append(pref.rank_positions_ref(scores[u], train[u].indices if train is not None else [], t))
    return np.concatenate([[0], np.cumsum([len(r) for r in rows])]), np.concatenate(idx), rows


def _by_rank(model, held_out, train, users):
    """The parent's route: rank() of the unseen items and a look-up."""
    rows = []
    for u in users:
        unseen = np.delete(np.arange(N_ITEMS), train[u].indices) if train is not None else np.arange(N_ITEMS)
        place = np.full(N_ITEMS, pref.SEEN, dtype=np.int64)
        if len(unseen):
            order = model.rank(unseen, int(u), topn=None)
            place[order] = np.arange(len(order))
        rows.append(place[np.unique(held_out[u].indices)])
    return rows


def _same(a, b):
    return sorted(a) == sorted(b) and all(a[k] == pytest.approx(b[k], rel=1e-12, abs=0) for k in b)   # (float64 sums in two orders)


@pytest.mark.parametrize("with_train", (True, False))
def test_rank_positions_is_the_reference_and_the_loop_over_rank(model, scores, held_out, train, with_train):
    tr = train if with_train else None
    users = np.flatnonzero(np.diff(held_out.indptr))
    assert 5 not in users and 6 in users
    indptr, indices, ranks, sc = model.rank_positions(held_out, exclude=tr, return_scores=True)
    want_ptr, want_idx, want_rows = _want(scores, held_out, tr, users)
    assert ranks.dtype == np.int64 and sc.dtype == np.float32 and indptr.dtype == np.int64
    assert np.array_equal(indptr, want_ptr) and np.array_equal(indices, want_idx)
    assert np.array_equal(ranks, np.concatenate(want_rows))
    assert ranks.min() >= pref.SEEN                                 # the caller never sees WMF_RANKPOS_BEYOND
    assert np.array_equal(ranks, np.concatenate(_by_rank(model, held_out, tr, users)))
    assert np.array_equal(sc.astype(np.int64), scores[np.repeat(users, np.diff(indptr)), indices])
    assert len(model.rank_positions(held_out, exclude=tr)) == 3
    if with_train:
        row7 = slice(indptr[list(users).index(7)], indptr[list(users).index(7) + 1])
        assert (ranks[row7] == pref.SEEN).all() and (ranks == pref.SEEN).sum() >= row7.stop - row7.start + 5
    else:
        assert (ranks >= 0).all()
    got = model.eval_ranking(held_out, train_mat=tr, topn=TOPN)
    assert _same(got, pref.ranking_metrics_ref(want_rows, TOPN))
    assert got[f"Recall@{N_ITEMS}"] == pytest.approx((ranks >= 0).mean(), rel=1e-12) and 0 < got["NDCG@10"] < 1


def test_users_subset_negative_indices_and_an_empty_row(model, scores, held_out, train):
    sub = [3, -1, 5, 6, -N_USERS, 3]
    resolved = [3, N_USERS - 1, 5, 6, 0, 3]
    indptr, indices, ranks = model.rank_positions(held_out, exclude=train, users=sub)
    want_ptr, want_idx, want_rows = _want(scores, held_out, train, resolved)
    assert np.array_equal(indptr, want_ptr) and np.array_equal(indices, want_idx) and np.array_equal(ranks, np.concatenate(want_rows))
    assert indptr[3] == indptr[2]                                   # user 5: no entries
    assert _same(model.eval_ranking(held_out, train, TOPN, users=sub), pref.ranking_metrics_ref(want_rows, TOPN))
    empty = model.rank_positions(held_out, exclude=train, users=[5])
    assert empty[0].tolist() == [0, 0] and len(empty[1]) == len(empty[2]) == 0


def test_rank_positions_in_small_batches(model, held_out, train, monkeypatch):
    from recmodel_amd import wmf_model
    want = model.rank_positions(held_out, exclude=train, return_scores=True)
    monkeypatch.setattr(wmf_model, "RECOMMEND_BATCH_USERS", 16)     # user 6 alone is 7 device rows: a batch ends inside it
    got = model.rank_positions(held_out, exclude=train, return_scores=True)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    monkeypatch.setattr(wmf_model, "RECOMMEND_BATCH_USERS", 1)
    assert np.array_equal(model.rank_positions(held_out, exclude=train)[2], want[2])


def test_unsorted_and_duplicated_input_is_canonicalised_on_copies(model, held_out, train):
    want = model.rank_positions(held_out, exclude=train)
    messy = []
    for m in (held_out, train):
        coo = m.tocoo()
        messy.append(sp.coo_matrix((np.concatenate([coo.data, coo.data])[::-1] / 2, (np.concatenate([coo.row, coo.row])[::-1],
                                                                                 np.concatenate([coo.col, coo.col])[::-1])), shape=m.shape))
    backwards = held_out.copy()                                     # CSR with every row's entries in descending order
    for u in range(N_USERS):
        row = slice(backwards.indptr[u], backwards.indptr[u + 1])
        backwards.indices[row], backwards.data[row] = held_out.indices[row][::-1], held_out.data[row][::-1]
    backwards.has_sorted_indices = False
    assert (np.diff(backwards.indices[backwards.indptr[6]:backwards.indptr[7]]) < 0).all()
    assert all(np.array_equal(a, b) for a, b in zip(model.rank_positions(backwards, exclude=train), want))
    assert (np.diff(backwards.indices[backwards.indptr[6]:backwards.indptr[7]]) < 0).all()      # ... and is left as it was
    keep = [(m.data.copy(), m.row.copy(), m.col.copy()) for m in messy]
    got = model.rank_positions(messy[0], exclude=messy[1])
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    for (data, row, col), m in zip(keep, messy):
        assert np.array_equal(m.data, data) and np.array_equal(m.row, row) and np.array_equal(m.col, col)
    before = (held_out.data.copy(), held_out.indices.copy(), held_out.indptr.copy())
    assert _same(model.eval_ranking(messy[0], messy[1], TOPN), model.eval_ranking(held_out, train, TOPN))
    assert all(np.array_equal(a, b) for a, b in zip(before, (held_out.data, held_out.indices, held_out.indptr)))


def test_device_hook_and_rank_fallback_agree(model, held_out, train):
    """eval_ranking through wmf_rank_positions and through the loop over WMF.rank on the same model."""
    from recmodel_amd import RecModel, WMF
    assert WMF._rank_positions is not RecModel._rank_positions

    class ByRank(WMF):
        _rank_positions = RecModel._rank_positions                  # no hook: eval_ranking asks rank() user by user
    slow = ByRank.__new__(ByRank)
    slow.__dict__.update(model.__dict__)
    for tr in (train, None):
        a, b = model.eval_ranking(held_out, tr, TOPN), slow.eval_ranking(held_out, tr, TOPN)
        assert a == b and sorted(a) == sorted(f"{m}@{k}" for m in ("Recall", "Precision", "ARHR", "NDCG") for k in TOPN)


def test_argument_errors_come_before_the_gpu(model, held_out, train, monkeypatch):
    from recmodel_amd import _lib

    def no_gpu():
        raise AssertionError("the GPU was asked for")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    with pytest.raises(ValueError):
        model.rank_positions(held_out.toarray())
    with pytest.raises(ValueError):
        model.rank_positions(held_out[:, :-1])
    with pytest.raises(ValueError):
        model.rank_positions(held_out, exclude=train.T.tocsr())
    with pytest.raises(IndexError):
        model.rank_positions(held_out, exclude=train, users=[N_USERS])
    with pytest.raises(IndexError):
        model.rank_positions(held_out, users=[-N_USERS - 1])
    with pytest.raises(ValueError):
        model.eval_ranking(held_out, train, topn=[10])
    with pytest.raises(ValueError):
        model.eval_ranking(held_out, train[:-1], topn=TOPN)
