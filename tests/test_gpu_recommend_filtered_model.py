"""The catalogue filters of WMF.recommend, recommend_for, similar_items and similar_users on the device: ``allow`` as a bool mask,
as a list of ids and as per-row masks with ``allow_idx``, against the routes they replace -- the complement added to ``exclude``
(bit for bit) and the loop over rank() of the allowed unseen items.  EXACT-class factors (tests/serving_ref.py): integer scores and
real ties, so every comparison of recommendations is for equality."""
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
    return sp.csr_matrix(t)


@pytest.fixture(scope="module")
def mask():
    m = np.random.default_rng(11).random(N_ITEMS) < 0.2
    m[[0, 1, N_ITEMS - 1]] = True
    return m


def _with_complement(train, masks):
    """train with the ineligible items of masks[u] added to row u."""
    return sp.csr_matrix(((train != 0).toarray() | ~masks).astype(np.float32))


def _by_rank(model, train, users, masks, topn):
    out = np.full((len(users), topn), -1, dtype=np.int64)
    for j, u in enumerate(users):
        cand = np.setdiff1d(np.flatnonzero(masks[j]), train[u].indices)
        best = model.rank(cand, int(u), topn) if len(cand) else cand
        out[j, :len(best)] = best
    return out


def _same(a, b):
    return all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b)) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))


@pytest.mark.parametrize("topn", (1, 10, 128))
def test_mask_list_exclude_and_rank_agree(model, train, mask, topn):
    users = list(range(N_USERS)) + [3, 3]
    by_mask = model.recommend(users, topn, exclude=train, return_scores=True, allow=mask)
    by_list = model.recommend(users, topn, exclude=train, return_scores=True, allow=np.flatnonzero(mask))
    by_exclude = model.recommend(users, topn, exclude=_with_complement(train, np.tile(mask, (N_USERS, 1))), return_scores=True)
    assert by_mask[0].dtype == np.int64 and by_mask[0].shape == (len(users), topn) and by_mask[1].dtype == np.float32
    assert _same(by_mask, by_list) and _same(by_mask, by_exclude)
    assert np.array_equal(by_mask[0], _by_rank(model, train, users, np.tile(mask, (len(users), 1)), topn))
    assert (by_mask[0][7] == -1).all() and (by_mask[1][7] == -np.inf).all()
    assert set(by_mask[0][8, :2]) <= {0, 1} and (by_mask[0][8, 2:] == -1).all()      # user 8 has two items left, both allowed


def test_ids_in_any_order_an_int_user_and_an_empty_list(model, train, mask):
    ids = np.flatnonzero(mask)
    shuffled = np.random.default_rng(5).permutation(np.concatenate([ids, ids[:7], ids[-3:] - N_ITEMS]))
    want = model.recommend(np.arange(N_USERS), 10, exclude=train, return_scores=True, allow=mask)
    assert _same(model.recommend(np.arange(N_USERS), 10, exclude=train, return_scores=True, allow=shuffled), want)
    assert _same(model.recommend(np.arange(N_USERS), 10, exclude=train, return_scores=True, allow=shuffled.tolist()), want)
    row = model.recommend(5, 10, exclude=train, allow=mask)
    assert row.shape == (10,) and np.array_equal(row, want[0][5])
    items, scores = model.recommend(-1, 4, return_scores=True, allow=ids)
    assert items.shape == scores.shape == (4,) and mask[items].all()
    for empty in ([], np.zeros(0, dtype=np.int64)):
        items, scores = model.recommend([1, 2], 3, exclude=train, return_scores=True, allow=empty)
        assert (items == -1).all() and items.shape == (2, 3) and (scores == -np.inf).all()
    assert (model.recommend([1, 2], 3, allow=np.zeros(N_ITEMS, dtype=bool)) == -1).all()
    assert (model.similar_items([1, 2], 3, allow=[]) == -1).all()


def test_per_row_masks_and_a_batch_boundary_inside_them(model, train, monkeypatch):
    from recmodel_amd import wmf_model
    rng = np.random.default_rng(17)
    shelves = rng.random((4, N_ITEMS)) < 0.25
    users = np.array([3, 3, 3, 3, 3] + list(range(N_USERS)))               # user 3 on every shelf, and unrestricted
    allow_idx = np.arange(len(users)) % 5 - 1
    allow_idx[:5] = [0, 1, 2, 3, -1]
    masks = np.where(allow_idx[:, None] < 0, True, shelves[allow_idx])
    want = _by_rank(model, train, users, masks, 10)
    got = model.recommend(users, 10, exclude=train, return_scores=True, allow=shelves, allow_idx=allow_idx)
    assert np.array_equal(got[0], want) and len({tuple(r) for r in got[0][:5]}) == 5
    for g in range(4):
        rows = np.flatnonzero(allow_idx == g)
        assert _same([a[rows] for a in got], model.recommend(users[rows], 10, exclude=train, return_scores=True, allow=shelves[g]))
    rows = np.flatnonzero(allow_idx == -1)
    assert _same([a[rows] for a in got], model.recommend(users[rows], 10, exclude=train, return_scores=True))
    monkeypatch.setattr(wmf_model, "RECOMMEND_BATCH_USERS", 3)
    assert _same(model.recommend(users, 10, exclude=train, return_scores=True, allow=shelves, allow_idx=allow_idx), got)
    assert _same(model.recommend(users, 10, exclude=train, return_scores=True, allow=np.flatnonzero(shelves[0])),
                 model.recommend(users, 10, exclude=train, return_scores=True, allow=shelves[0]))


def test_beyond_the_fused_maximum_with_a_filter(model, train):
    big = np.random.default_rng(19).random(N_ITEMS) < 0.8
    users = [0, 7, 8, 21]
    masks = np.tile(big, (len(users), 1))
    got, scores = model.recommend(users, 200, exclude=train, return_scores=True, allow=big)
    assert got.shape == (4, 200) and np.array_equal(got, _by_rank(model, train, users, masks, 200))
    assert np.array_equal(got, model.recommend(users, 200, exclude=train, allow=np.flatnonzero(big)))
    assert np.array_equal(got[:, :128], model.recommend(users, 128, exclude=train, allow=big))
    valid = got >= 0
    assert (scores[~valid] == -np.inf).all() and big[got[valid]].all() and (~valid).any()
    shelves = np.stack([big, ~big])
    per_row = model.recommend(users, 200, exclude=train, allow=shelves, allow_idx=[0, 1, -1, 1])
    assert np.array_equal(per_row, _by_rank(model, train, users, np.stack([big, ~big, np.ones(N_ITEMS, dtype=bool), ~big]), 200))


def test_recommend_for_keeps_its_identity_under_a_filter(model, mask):
    from recmodel_amd import WMF
    counts = sp.random(9, N_ITEMS, density=0.1, format="csr", random_state=4, dtype=np.float32)
    counts.data[:] = np.ceil(counts.data * 5)
    folded = WMF(num_items=N_ITEMS, num_users=9, dim=F - 1, gamma=0.1, weighted=True, bias=True)
    folded.users, folded.items = model.fold_in(counts), model.items
    shelves = np.stack([mask, ~mask])
    allow_idx = np.arange(9) % 3 - 1
    for kw in (dict(allow=mask), dict(allow=np.flatnonzero(mask)), dict(allow=shelves, allow_idx=allow_idx)):
        got = model.recommend_for(counts, 10, return_scores=True, **kw)
        assert _same(got, folded.recommend(np.arange(9), 10, exclude=counts, return_scores=True, **kw)), list(kw)
        eligible = np.where(allow_idx[:, None] < 0, True, shelves[allow_idx]) if "allow_idx" in kw else np.tile(mask, (9, 1))
        assert all(eligible[b, got[0][b]].all() for b in range(9))
    assert (model.recommend_for(counts, 10, allow=[]) == -1).all()


@pytest.mark.parametrize("side", ("items", "users"))
@pytest.mark.parametrize("metric", ("dot", "cosine"))
def test_similar_under_a_filter_against_float64(side, metric):
    """ROUNDED-class factors (no ties): the neighbours among the allowed rows by float64 NumPy."""
    from recmodel_amd import WMF
    m = WMF(num_items=N_ITEMS, num_users=N_USERS, dim=F - 1, gamma=0.1, weighted=True, bias=True)
    m.users, m.items = ref.rounded_factors(N_USERS, F, 71), ref.rounded_factors(N_ITEMS, F, 72)
    M = getattr(m, side).astype(np.float64)[:, 1:]                   # the bias column is no feature
    n = len(M)
    if metric == "cosine":
        M = M / np.linalg.norm(M, axis=1, keepdims=True)
    rng = np.random.default_rng(23)
    allowed = rng.random(n) < 0.4
    q = np.array([0, n - 1, 5, 5, 17])
    allowed[q[:3]] = True
    S = M[q] @ M.T

    def want(masks, topn):
        out = np.full((len(q), topn), -1, dtype=np.int64)
        for b in range(len(q)):
            s = np.where(masks[b], S[b], -np.inf)
            s[q[b]] = -np.inf
            best = np.argsort(-s, kind="stable")[:topn]
            best = best[np.isfinite(s[best])]
            out[b, :len(best)] = best
        return out
    call = m.similar_items if side == "items" else m.similar_users
    got, scores = call(q, 10, metric=metric, return_scores=True, allow=allowed)
    assert np.array_equal(got, want(np.tile(allowed, (len(q), 1)), 10))
    assert np.allclose(scores, np.take_along_axis(S, got, axis=1), rtol=1e-5, atol=1e-6)
    ids = np.flatnonzero(allowed)
    by_ids = call(q, 10, metric=metric, return_scores=True, allow=ids[::-1])
    assert np.array_equal(by_ids[0], got) and np.array_equal(by_ids[1].view(np.int32), scores.view(np.int32))
    two = np.stack([allowed, ~allowed])
    idx = np.array([0, 1, -1, 1, 0])
    assert np.array_equal(call(q, 10, metric=metric, allow=two, allow_idx=idx), want(np.where(idx[:, None] < 0, True, two[idx]), 10))
    few = call(q, 10, metric=metric, allow=[int(q[0]), int(q[2]), 3])     # fewer allowed rows than topn; the row itself is left out
    assert np.array_equal(few, want(np.tile(np.isin(np.arange(n), [q[0], q[2], 3]), (len(q), 1)), 10)) and (few[0] != q[0]).all()
