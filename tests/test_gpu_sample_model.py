"""WMF.sample_items, WMF.sample_items_for and WMF.log_partition on small trained models (k = 16, and k = 128 + biases): temperature
zero against candidates(), the filters, sample_items_for against sample_items on a model whose users are fold_in(count_rows), the
independence of a user's list from the batch, the log-probabilities against float64 NumPy on predict()'s scores, and the first-pick
frequencies against softmax(predict / T)."""
import math

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.stats

import sample_ref as sref
import serving_ref as ref

pytestmark = pytest.mark.gpu

N_USERS, N_ITEMS = 300, 600
MODELS = {"k16": (16, False), "k128-bias": (128, True)}
USERS = np.array([0, 1, 2, 3, 17, 17, 101, 250, N_USERS - 1, -2])


@pytest.fixture(scope="module")
def train_mat():
    from recmodel_amd import synth
    indptr, indices, counts = synth.make_counts(N_USERS, N_ITEMS, 9, seed=5)
    return synth.to_scipy(indptr, indices, counts, (N_USERS, N_ITEMS)).astype(np.float64)


@pytest.fixture(scope="module", params=list(MODELS))
def model(request, train_mat):
    from recmodel_amd import WMF
    dim, bias = MODELS[request.param]
    m = WMF(num_items=N_ITEMS, num_users=N_USERS, dim=dim, gamma=0.1, weighted=True, bias=bias)
    m.train(utility_mat=train_mat, iterations=2, eval_mat=train_mat, count_mat=train_mat, cores=1)
    return m


def _bits(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))


def test_temperature_zero_is_candidates(model, train_mat):
    mask = np.random.default_rng(1).random(N_ITEMS) < 0.3
    for kw in ({}, dict(exclude=train_mat), dict(exclude=train_mat, allow=mask), dict(allow=np.flatnonzero(mask))):
        for n in (1, 10, 200):
            want = model.candidates(USERS, n, return_scores=True, **kw)
            for seed in (0, 99):
                got = model.sample_items(USERS, n, temperature=0, seed=seed, return_scores=True, **kw)
                assert got[0].dtype == np.int64 and got[1].dtype == np.float32 and _bits(got, want), (n, seed, list(kw))
    assert np.array_equal(model.sample_items(5, 10, temperature=0), model.candidates(5, 10))


def test_picks_respect_the_filters_and_never_repeat(model, train_mat):
    rng = np.random.default_rng(2)
    shelves = rng.random((3, N_ITEMS)) < 0.4
    allow_idx = np.arange(len(USERS)) % 4 - 1
    rows = np.where(USERS < 0, USERS + N_USERS, USERS)
    for T in (0.5, 5.0):
        items, scores = model.sample_items(USERS, 50, temperature=T, seed=3, exclude=train_mat, allow=shelves, allow_idx=allow_idx, return_scores=True)
        assert items.shape == (len(USERS), 50) and (items >= 0).all()
        for b, u in enumerate(rows):
            assert len(set(items[b])) == 50 and not set(items[b]) & set(train_mat[u].indices)
            assert allow_idx[b] < 0 or shelves[allow_idx[b], items[b]].all()
        uu = np.repeat(rows, 50)
        assert np.abs(scores.ravel() - model.predict(uu, items.ravel())).max() <= 1e-4 * max(1.0, np.abs(scores).max())
    ids = np.sort(rng.choice(N_ITEMS, 30, replace=False))
    few = model.sample_items(USERS, 50, temperature=1.0, allow=ids)
    assert (np.sort(few[:, :30], axis=1) == ids).all() and (few[:, 30:] == -1).all()
    assert (model.sample_items(USERS, 5, allow=[]) == -1).all()
    assert model.sample_items([], 5).shape == (0, 5)


def test_the_list_of_a_user_does_not_depend_on_the_batch(model, train_mat, monkeypatch):
    from recmodel_amd import wmf_model
    users = np.arange(40)
    want = model.sample_items(users, 20, temperature=1.0, seed=11, exclude=train_mat, return_scores=True)
    one = model.sample_items([7], 20, temperature=1.0, seed=11, exclude=train_mat, return_scores=True)
    assert _bits(one, [a[7: 8] for a in want])
    back = model.sample_items(users[::-1], 20, temperature=1.0, seed=11, exclude=train_mat, return_scores=True)
    assert _bits(back, [a[::-1] for a in want])
    twice = model.sample_items([7, 7], 20, temperature=1.0, seed=11, exclude=train_mat)
    assert np.array_equal(twice[0], twice[1]) and np.array_equal(twice[0], want[0][7])      # the stream is the user id
    two = model.sample_items([7, 7], 20, temperature=1.0, seed=11, exclude=train_mat, streams=[7, 8])
    assert np.array_equal(two[0], want[0][7]) and not np.array_equal(two[0], two[1])
    monkeypatch.setattr(wmf_model, "RECOMMEND_BATCH_USERS", 3)
    assert _bits(model.sample_items(users, 20, temperature=1.0, seed=11, exclude=train_mat, return_scores=True), want)
    monkeypatch.setattr(wmf_model, "RECOMMEND_BATCH_USERS", 4096)
    other = model.sample_items(users, 20, temperature=1.0, seed=12, exclude=train_mat)
    assert not np.array_equal(other, want[0]) and (other != want[0]).any(axis=1).all()      # another seed, another list


def _counts(B):
    counts = sp.random(B, N_ITEMS, density=0.03, format="lil", random_state=4, dtype=np.float32)
    counts[1, :] = 0.0                                                # an empty history
    counts = sp.csr_matrix(counts)
    counts.eliminate_zeros()
    counts.data[:] = np.ceil(counts.data * 5)
    return counts


def test_sample_items_for_is_sample_items_on_the_folded_in_rows(model):
    from recmodel_amd import WMF
    B = 9
    counts = _counts(B)
    bias = model.bias is True
    dim = model.items.shape[1] - int(bias)
    folded = WMF(num_items=N_ITEMS, num_users=B, dim=dim, gamma=0.1, weighted=True, bias=bias)
    folded.users, folded.items = model.fold_in(counts), model.items
    assert folded.users.shape[1] == model.items.shape[1]
    mask = np.random.default_rng(12).random(N_ITEMS) < 0.3
    streams = np.arange(B, dtype=np.uint64) + np.uint64(2 ** 63)
    for kw in ({}, dict(allow=mask), dict(allow=np.flatnonzero(mask))):
        got = model.sample_items_for(counts, 40, temperature=2.0, seed=5, streams=streams, return_scores=True, return_log_prob=True, **kw)
        want = folded.sample_items(np.arange(B), 40, temperature=2.0, seed=5, streams=streams, exclude=counts, return_scores=True,
                                   return_log_prob=True, **kw)
        assert _bits(got, want) and np.array_equal(got[2], want[2]), list(kw)
        for b in range(B):
            assert not set(counts[b].indices) & set(got[0][b])
    # the default stream is the position in count_rows -- and on a model of B users that is the user id
    assert np.array_equal(model.sample_items_for(counts, 40, seed=5), folded.sample_items(np.arange(B), 40, seed=5, exclude=counts))
    assert model.sample_items_for(sp.csr_matrix((0, N_ITEMS)), 7).shape == (0, 7)


def test_a_failed_row_has_no_sample():
    from recmodel_amd import WMF
    n = 400
    m = WMF(num_items=n, num_users=3, dim=8, gamma=0.1, weighted=True)
    m.items = np.zeros((n, 8), dtype=np.float32)
    m.items[np.arange(n), np.arange(n) % 8] = 1.0
    m.users = np.zeros((3, 8), dtype=np.float32)
    rows = sp.csr_matrix((np.array([400.0, 0.1]), np.array([3, 5]), np.array([0, 1, 1, 2])), shape=(3, n))
    items, scores, logp = m.sample_items_for(rows, 20, return_scores=True, return_log_prob=True, alpha=-3, pre_process_count="linear")
    assert (items[0] == -1).all() and np.isneginf(scores[0]).all() and np.isneginf(logp[0]).all()
    assert (items[1:] >= 0).all() and (scores[1] == 0).all() and 5 not in items[2]
    assert np.allclose(logp[1], -math.log(n), atol=1e-5)             # an all-zero row: the uniform draw


def test_log_probabilities_against_numpy_on_predict(model, train_mat):
    """logp = score / T - log Z.  Reference: float64 NumPy on predict()'s float32 scores.  The gate: wmf_log_partition's
    (include/wmf_hip.h) with 2 B for B -- the scan's score and predict()'s are each within B, serving_ref.score_bound, of the exact
    one -- plus the same 2 B / T and one rounding for the pick's own score / T."""
    rows = np.where(USERS < 0, USERS + N_USERS, USERS)
    bias = int(model.bias is True)
    Uf, If = model.users.astype(np.float32), model.items.astype(np.float32)
    everything = np.arange(N_ITEMS)
    mask = np.random.default_rng(3).random(N_ITEMS) < 0.5
    worst = 0.0
    for T in (0.5, 3.0):
        T32 = float(np.float32(T))
        for kw in (dict(exclude=train_mat), dict(allow=mask)):
            items, scores, logp = model.sample_items(USERS, 30, temperature=T, seed=4, return_scores=True, return_log_prob=True, **kw)
            logz = model.log_partition(USERS, temperature=T, **kw)
            assert logp.dtype == np.float64 and logz.dtype == np.float32 and logz.shape == (len(USERS),)
            assert np.array_equal(logp, scores.astype(np.float64) / np.float64(np.float32(T)) - logz.astype(np.float64)[:, None])
            for b, u in enumerate(rows):
                keep = mask.copy() if "allow" in kw else np.ones(N_ITEMS, dtype=bool)
                if "exclude" in kw:
                    keep[train_mat[u].indices] = False
                pred = model.predict(np.full(N_ITEMS, u), everything).astype(np.float64)
                B = float(ref.score_bound(Uf, If, np.full(N_ITEMS, u), everything, bias)[keep].max())
                L64 = sref.logsumexp64(pred[keep] / T32)
                gate = 2 * B / T32 + 4 * 2.0 ** -23 * (2 + math.log(keep.sum())) + 2.0 ** -23 * abs(L64)
                assert abs(float(logz[b]) - L64) <= gate, (T, list(kw), b)
                want = pred[items[b]] / T32 - L64
                pick_gate = gate + 2 * B / T32 + 2.0 ** -23 * np.abs(pred[items[b]] / T32)
                ratio = float((np.abs(logp[b] - want) / pick_gate).max())
                worst = max(worst, ratio)
                assert ratio <= 1.0, (T, list(kw), b, ratio)
                assert (logp[b] < 0).all()
    print(f"log-probabilities: worst error / gate = {worst:.4f}")
    assert model.log_partition(5, temperature=1.0).shape == ()
    with pytest.raises(ValueError, match="temperature"):
        model.sample_items(USERS, 5, temperature=0, return_log_prob=True)


def test_first_pick_frequencies_at_a_large_temperature(model):
    """One user under streams 0 .. 4095 on a 64-item allow list: the first picks against softmax(predict / T), T twice the spread of
    the scores, so that every cell expects at least 5; the 1 - 10^-6 quantile at 63 degrees of freedom."""
    user, streams = 17, np.arange(4096)
    ids = np.sort(np.random.default_rng(5).choice(N_ITEMS, 64, replace=False))
    pred = model.predict(np.full(64, user), ids).astype(np.float64)
    T = 2.0 * max(float(np.ptp(pred)), 0.5)
    picks = model.sample_items(np.full(4096, user), 1, temperature=T, seed=6, allow=ids, streams=streams)[:, 0]
    assert np.isin(picks, ids).all()
    expected = 4096 * sref.plackett_luce_first(pred, float(np.float32(T)))
    assert expected.min() >= 5
    stat, cells = sref.chi_square(np.bincount(np.searchsorted(ids, picks), minlength=64), expected)
    print(f"first picks at T = {T:.3f}: chi-square {stat:.1f} over {cells} cells")
    assert cells == 64 and stat < scipy.stats.chi2.ppf(1 - 1e-6, 63)
