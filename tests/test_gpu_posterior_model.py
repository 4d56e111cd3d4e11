"""WMF.posterior_draws, recommend_thompson[_for], score_posterior and recommend_ucb_for on small trained models (k = 16, and
k = 128 with biases): the three identities bit for bit (sigma = 0 is fold_in / recommend_for, c = 0 is recommend_for, a Thompson
list is recommend on the drawn rows), independence of how the batch is cut, score_posterior against float64 NumPy on the model's
factors, recommend_ucb_for against the host restatement on the device's own pool, scores and variances with its tie rule, the
filters and the history's exclusion, failed and empty histories."""
import numpy as np
import pytest
import scipy.sparse as sp

import posterior_ref as ref
from conftest import record_error

pytestmark = pytest.mark.gpu

N_USERS, N_ITEMS = 300, 600
GAMMA = 0.1
MODELS = {"k16": (16, False), "k128-bias": (128, True)}
USERS = np.array([0, 1, 2, 3, 17, 17, 101, 250, N_USERS - 1, N_USERS - 2])


@pytest.fixture(scope="module")
def train_mat():
    from recmodel_amd import synth
    indptr, indices, counts = synth.make_counts(N_USERS, N_ITEMS, 9, seed=5)
    return synth.to_scipy(indptr, indices, counts, (N_USERS, N_ITEMS)).astype(np.float64)


@pytest.fixture(scope="module", params=list(MODELS))
def model(request, train_mat):
    from recmodel_amd import WMF
    dim, bias = MODELS[request.param]
    m = WMF(num_items=N_ITEMS, num_users=N_USERS, dim=dim, gamma=GAMMA, weighted=True, bias=bias)
    m.train(utility_mat=train_mat, iterations=2, eval_mat=train_mat, count_mat=train_mat)
    m.case_name = request.param
    return m


def _strangers(seed=9):
    """Histories that are rows of no training matrix: one of them empty, one with a stored zero."""
    rng = np.random.default_rng(seed)
    degrees = np.array([5, 0, 1, 30, 12, 2, 9])
    indptr = np.concatenate([[0], np.cumsum(degrees)])
    indices = np.concatenate([np.sort(rng.choice(N_ITEMS, d, replace=False)) for d in degrees]).astype(np.int32)
    counts = rng.integers(1, 8, len(indices)).astype(np.float64)
    counts[0] = 0.0
    return sp.csr_matrix((counts, indices, indptr), shape=(len(degrees), N_ITEMS))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _other(model, X):
    from recmodel_amd import WMF
    other = WMF(num_items=N_ITEMS, num_users=len(X), dim=model.dim, gamma=GAMMA, weighted=True, bias=model.bias)
    other.items = model.items
    other.users = np.ascontiguousarray(X)
    return other


def test_sigma_zero_and_c_zero_are_the_point_estimate(model, train_mat):
    for rows in (train_mat[USERS], _strangers()):
        B, f = rows.shape[0], model.items.shape[1]
        X = model.fold_in(rows)
        D = model.posterior_draws(rows, draws=3, sigma=0, seed=5)
        assert D.dtype == np.float32 and D.shape == (B, 3, f)
        for s in range(3):
            assert np.array_equal(_bits(D[:, s]), _bits(X))
        items, scores = model.recommend_for(rows, 7, return_scores=True)
        t_items, t_scores = model.recommend_thompson_for(rows, 7, sigma=0, seed=3, return_scores=True)
        assert t_items.dtype == np.int64 and np.array_equal(t_items, items) and np.array_equal(_bits(t_scores), _bits(scores))
        assert np.array_equal(model.recommend_thompson_for(rows, 7, sigma=0), items)
        u_items, u_scores, u_std = model.recommend_ucb_for(rows, 7, pool=50, c=0, return_scores=True, return_std=True)
        assert u_items.dtype == np.int64 and np.array_equal(u_items, items) and np.array_equal(_bits(u_scores), _bits(scores))
        assert u_std.dtype == np.float32 and (u_std > 0).all()
        assert np.array_equal(model.recommend_ucb_for(rows, 7, c=0), items)
        assert np.array_equal(model.recommend_ucb_for(rows, 7, pool=7, c=0, exclude_history=False), model.recommend_for(rows, 7, exclude_history=False))
    assert model.posterior_draws(sp.csr_matrix((0, N_ITEMS)), 4).shape == (0, 4, f)
    assert model.recommend_thompson_for(sp.csr_matrix((0, N_ITEMS)), 3).shape == (0, 3)
    assert model.recommend_ucb_for(sp.csr_matrix((0, N_ITEMS)), 3).shape == (0, 3)
    assert model.score_posterior(sp.csr_matrix((0, N_ITEMS)), np.zeros((0, 2), dtype=np.int64))[0].shape == (0, 2)


def test_thompson_is_recommend_on_the_drawn_rows(model, train_mat):
    rows = train_mat[USERS]
    B = rows.shape[0]
    streams = np.arange(B) + 1000                                    # (USERS lists user 17 twice: two streams, two draws)
    for topn in (7, 200):                                            # 200: beyond RECOMMEND_MAX_TOPN, the wide scan
        X = model.posterior_draws(rows, draws=1, sigma=1.0, seed=11, streams=streams)[:, 0]
        assert np.isfinite(X).all() and not np.array_equal(X, model.fold_in(rows)) and not np.array_equal(X[4], X[5])
        items, scores = model.recommend_thompson_for(rows, topn, sigma=1.0, seed=11, streams=streams, return_scores=True)
        want, want_scores = _other(model, X).recommend(np.arange(B), topn, exclude=rows, return_scores=True)
        assert np.array_equal(items, want) and np.array_equal(_bits(scores), _bits(want_scores))
        for b in range(B):
            assert not np.isin(items[b], rows[b].indices).any()
        free = model.recommend_thompson_for(rows, topn, sigma=1.0, seed=11, streams=streams, exclude_history=False)
        assert np.array_equal(free, _other(model, X).recommend(np.arange(B), topn))
    # the draws of a longer call start with the shorter one's, and sigma scales the deviation from the fold-in
    D = model.posterior_draws(rows, draws=20, sigma=1.0, seed=11, streams=streams)
    assert np.array_equal(_bits(D[:, 0]), _bits(X))
    half = model.posterior_draws(rows, draws=1, sigma=0.5, seed=11, streams=streams)[:, 0]
    mean = model.fold_in(rows).astype(np.float64)
    assert np.abs((half - mean) * 2 - (X - mean)).max() <= 1e-4 * np.abs(X - mean).max()
    # exploration is wider for the shorter history: the total deviation of 200 draws, a row of 1 entry against one of 30
    S = _strangers()
    spread = model.posterior_draws(S, draws=200, sigma=1.0, seed=2).astype(np.float64).std(axis=1).sum(axis=1)
    assert spread[2] > spread[3] and spread[1] > spread[3]


def test_a_users_thompson_list_does_not_depend_on_the_batch(model, train_mat, monkeypatch):
    from recmodel_amd import wmf_model
    users = np.arange(0, N_USERS, 9)
    items, scores = model.recommend_thompson(users, train_mat, 5, sigma=0.8, seed=4, return_scores=True)
    assert items.shape == (len(users), 5) and (items >= 0).all()
    one = model.recommend_thompson(int(users[3]), train_mat, 5, sigma=0.8, seed=4)
    assert one.shape == (5,) and np.array_equal(one, items[3])
    pair, pair_scores = model.recommend_thompson(users[[7, 3, 3]], train_mat, 5, sigma=0.8, seed=4, return_scores=True)
    assert np.array_equal(pair, items[[7, 3, 3]]) and np.array_equal(_bits(pair_scores), _bits(scores[[7, 3, 3]]))
    assert np.array_equal(model.recommend_thompson(users - N_USERS, train_mat, 5, sigma=0.8, seed=4), items)     # negative ids wrap
    # the thin form is recommend_thompson_for on the users' rows with the ids as streams, and the history is excluded
    want = model.recommend_thompson_for(train_mat[users], 5, sigma=0.8, seed=4, streams=users)
    assert np.array_equal(items, want)
    for b, u in enumerate(users):
        assert not np.isin(items[b], train_mat[int(u)].indices).any()
    assert not np.array_equal(model.recommend_thompson(users, train_mat, 5, sigma=0.8, seed=5), items)
    # batches that _scan_batches splits
    draws = model.posterior_draws(train_mat[users], draws=3, sigma=0.8, seed=4)
    tg = model.recommend_for(train_mat[users], 6)
    mean, var = model.score_posterior(train_mat[users], tg)
    ucb = model.recommend_ucb_for(train_mat[users], 5, pool=40, c=2.0, return_scores=True, return_std=True)
    monkeypatch.setattr(wmf_model, "RECOMMEND_BATCH_USERS", 3)
    assert len(users) % 3 != 0
    again, again_scores = model.recommend_thompson(users, train_mat, 5, sigma=0.8, seed=4, return_scores=True)
    assert np.array_equal(again, items) and np.array_equal(_bits(again_scores), _bits(scores))
    assert np.array_equal(_bits(model.posterior_draws(train_mat[users], draws=3, sigma=0.8, seed=4)), _bits(draws))
    m2, v2 = model.score_posterior(train_mat[users], tg)
    assert np.array_equal(_bits(m2), _bits(mean)) and np.array_equal(_bits(v2), _bits(var))
    for a, b in zip(model.recommend_ucb_for(train_mat[users], 5, pool=40, c=2.0, return_scores=True, return_std=True), ucb):
        assert np.array_equal(a, b)


def _float64_scores(model, rows, tg):
    """(mean, var, M) of tests/posterior_ref.py::scores64 on the numbers the device reads: float32 factors, float32 confidences."""
    Y32 = model.items.astype(np.float32)
    conf = (10 * np.log1p(rows.data.astype(np.float32).astype(np.float64))).astype(np.float32)
    return ref.scores64(Y32, int(model.bias is True), GAMMA, rows.indptr.astype(np.int64), rows.indices.astype(np.int32), conf,
                        np.asarray(tg, dtype=np.int32)), (Y32, conf)


def test_score_posterior_against_float64(model, train_mat, monkeypatch):
    from recmodel_amd import wmf_model
    rows = _strangers()
    B = rows.shape[0]
    rng = np.random.default_rng(3)
    tg = rng.integers(0, N_ITEMS, (B, 21))
    tg[:, 0], tg[:, 1], tg[:, 5], tg[:, 20] = 0, N_ITEMS - 1, -1, tg[:, 2]
    tg[0, 3] = rows[0].indices[0]
    mean, var = model.score_posterior(rows, tg)
    assert mean.dtype == var.dtype == np.float32 and mean.shape == var.shape == (B, 21)
    (m64, v64, M), (Y32, conf) = _float64_scores(model, rows, tg)
    bias = int(model.bias is True)
    W32 = ref.whitening(Y32, bias, GAMMA).astype(np.float32)
    m32, v32 = ref.restated_scores32(Y32, bias, W32, rows.indptr.astype(np.int64), rows.indices.astype(np.int32), conf, tg.astype(np.int32))
    live = tg >= 0
    for what, got, r32, want, scale in (("var", var, v32, v64, v64), ("mean", mean, m32, m64, M)):
        restated = np.where(live, ref.score_errors(r32, want, scale), 0.0)
        err = np.where(live, ref.score_errors(got, want, scale), 0.0)
        print(f"{model.case_name}: score_posterior {what} error {err.max():.3e}, restated {restated.max():.3e}")
        record_error("posterior_model", **{f"{model.case_name}_{what}": err.max(), f"{model.case_name}_{what}_restated": restated.max()})
        assert (err <= ref.gate_of(restated)).all(), (what, err.max())
    assert (mean[:, 5] == 0).all() and (var[:, 5] == 0).all() and (var >= 0).all()      # (an item nobody touched has zero factors)
    assert np.array_equal(_bits(var[:, 2]), _bits(var[:, 20])) and np.array_equal(_bits(mean[:, 2]), _bits(mean[:, 20]))
    # the mean is predict on the folded-in row; the variance of 2000 draws' scores is var
    X = model.fold_in(rows)
    Yt, beta = ref.tilde(Y32, bias)
    assert np.abs(mean - np.where(live, np.einsum("btf,bf->bt", Yt[np.maximum(tg, 0)], X.astype(np.float64)) + beta[np.maximum(tg, 0)], 0)).max() \
        <= 1e-4 * max(1.0, np.abs(m64).max())
    draws = model.posterior_draws(rows, draws=2000, sigma=1.0, seed=1).astype(np.float64)
    sample_var = np.einsum("btf,bdf->bdt", Yt[np.maximum(tg, 0)], draws).var(axis=1)
    assert (np.abs(sample_var - v64)[live] <= 6 * np.sqrt(2 / 2000) * v64[live]).all()
    # more targets than one call takes: split on the host, the same bits
    monkeypatch.setattr(wmf_model, "POSTERIOR_MAX_TARGETS", 8)
    m2, v2 = model.score_posterior(rows, tg)
    assert np.array_equal(_bits(m2), _bits(mean)) and np.array_equal(_bits(v2), _bits(var))


def _ucb_restated(pool_items, pool_scores, var, c, topn):
    """The host restatement of recommend_ucb_for's last step: key = score + c sqrt(var) in float32, the pool sorted by id, then a
    stable descending sort by key; padding (-1, -inf) last."""
    B = len(pool_items)
    items = np.full((B, topn), -1, dtype=np.int64)
    scores = np.full((B, topn), -np.inf, dtype=np.float32)
    std = np.zeros((B, topn), dtype=np.float32)
    for b in range(B):
        ok = pool_items[b] >= 0
        ids, s, sd = pool_items[b][ok], pool_scores[b][ok], np.sqrt(var[b][ok].astype(np.float32))
        key = (s + (np.float32(c) * sd).astype(np.float32)).astype(np.float32)
        by_id = np.argsort(ids, kind="stable")
        order = by_id[np.argsort(-key[by_id].astype(np.float64), kind="stable")][:topn]
        items[b, :len(order)], scores[b, :len(order)], std[b, :len(order)] = ids[order], s[order], sd[order]
    return items, scores, std


def test_ucb_against_the_host_restatement(model, train_mat):
    rows = train_mat[USERS]
    pool, topn = 60, 9
    pool_items, pool_scores = model.candidates_for(rows, pool, return_scores=True)
    _, var = model.score_posterior(rows, pool_items)
    base_std = None
    for c in (0.0, 1.0, 50.0):
        items, scores, std = model.recommend_ucb_for(rows, topn, pool=pool, c=c, return_scores=True, return_std=True)
        want = _ucb_restated(pool_items, pool_scores, var, c, topn)
        assert np.array_equal(items, want[0]) and np.array_equal(_bits(scores), _bits(want[1])) and np.array_equal(_bits(std), _bits(want[2]))
        i2, s2 = model.recommend_ucb_for(rows, topn, pool=pool, c=c, return_std=True)
        assert np.array_equal(i2, items) and np.array_equal(_bits(s2), _bits(std))
        assert np.array_equal(model.recommend_ucb_for(rows, topn, pool=pool, c=c), items)
        for b in range(len(USERS)):
            assert np.isin(items[b], pool_items[b]).all() and not np.isin(items[b], rows[b].indices).any()
        base_std = std if c == 0.0 else base_std
    # a large c strictly raises the mean std of the lists against c = 0, and changes them
    print(f"{model.case_name}: mean std of the lists, c = 0: {base_std.mean():.4f}, c = 50: {std.mean():.4f}")
    assert std.mean() > base_std.mean() and not np.array_equal(items, model.recommend_for(rows, topn))
    # pool = topn: the same set in another order
    items = model.recommend_ucb_for(rows, 9, pool=9, c=50.0)
    assert np.array_equal(np.sort(items, axis=1), np.sort(model.recommend_for(rows, 9), axis=1))


def test_ucb_ties_go_to_the_lower_id():
    """Unit vectors as items: every item off a row's history scores exactly 0 and has one prior variance, so at c = 0 -- and at any c
    -- the keys of those items are equal and the lists are in item order; the history's items score higher and come first."""
    from recmodel_amd import WMF
    m = WMF(num_items=40, num_users=3, dim=40, gamma=0.1, weighted=True)
    m.items = np.eye(40, dtype=np.float32)
    m.users = np.zeros((3, 40), dtype=np.float32)
    rows = sp.csr_matrix((np.array([1.0, 2.0, 3.0]), np.array([30, 7, 21]), np.array([0, 2, 2, 3])), shape=(3, 40))
    for c in (0.0, 3.0):
        items, scores, std = m.recommend_ucb_for(rows, 6, pool=25, c=c, exclude_history=False, return_scores=True, return_std=True)
        assert np.array_equal(items[1], np.arange(6)) and (scores[1] == 0).all() and len(set(std[1].tolist())) == 1
        if c == 0.0:
            assert np.array_equal(items[0], [30, 7, 0, 1, 2, 3]) or np.array_equal(items[0], [7, 30, 0, 1, 2, 3])
            assert np.array_equal(items[2], [21, 0, 1, 2, 3, 4])
            assert np.array_equal(items, m.recommend_for(rows, 6, exclude_history=False))
        else:                                                        # the unseen items are the uncertain ones: they overtake
            assert not np.isin(items[2], [21]).any() and np.array_equal(items[2], np.arange(6))
    assert np.array_equal(m.recommend_ucb_for(rows, 6, pool=25, c=0.0)[2], [0, 1, 2, 3, 4, 5])


def test_filters_pass_through(model, train_mat):
    rows = train_mat[USERS]
    B = rows.shape[0]
    allow = np.zeros(N_ITEMS, dtype=bool)
    allow[::3] = True
    ids = np.nonzero(allow)[0]
    masks = np.stack([allow, ~allow])
    idx = np.arange(B) % 3 - 1                                       # -1: unrestricted
    X = model.posterior_draws(rows, 1, sigma=1.0, seed=6)[:, 0]
    other = _other(model, X)
    for kw in (dict(allow=allow), dict(allow=ids), dict(allow=masks, allow_idx=idx)):
        items, scores = model.recommend_thompson_for(rows, 8, sigma=1.0, seed=6, return_scores=True, **kw)
        want, want_scores = other.recommend(np.arange(B), 8, exclude=rows, return_scores=True, **kw)
        assert np.array_equal(items, want) and np.array_equal(_bits(scores), _bits(want_scores))
        ucb = model.recommend_ucb_for(rows, 8, pool=30, c=0, **kw)
        assert np.array_equal(ucb, model.recommend_for(rows, 8, **kw))
        ucb = model.recommend_ucb_for(rows, 8, pool=30, c=5.0, **kw)
        pool_items = model.candidates_for(rows, 30, **kw)
        for b in range(B):
            assert np.isin(ucb[b], pool_items[b]).all() and not np.isin(ucb[b][ucb[b] >= 0], rows[b].indices).any()
        if "allow_idx" not in kw:
            assert allow[items].all() and allow[ucb].all()
    few = np.array([5, 9, 400])                                      # fewer eligible items than topn: padding
    items, scores, std = model.recommend_ucb_for(rows, 5, pool=10, c=1.0, allow=few, exclude_history=False, return_scores=True, return_std=True)
    assert (np.sort(items[:, :3], axis=1) == few).all() and (items[:, 3:] == -1).all() and np.isneginf(scores[:, 3:]).all() and (std[:, 3:] == 0).all()
    assert (model.recommend_thompson_for(rows, 5, allow=np.zeros(0, dtype=np.int64)) == -1).all()
    assert (model.recommend_ucb_for(rows, 5, allow=np.zeros(0, dtype=np.int64)) == -1).all()


def test_failed_and_empty_histories():
    """tests/test_gpu_foldin_model.py's model: unit vectors as items, alpha = -3 gives row 0 an indefinite system; row 1 is empty;
    row 2 (weight -0.3) is solved."""
    from recmodel_amd import WMF
    m = WMF(num_items=8, num_users=3, dim=8, gamma=0.1, weighted=True)
    m.items = np.eye(8, dtype=np.float32)
    m.users = np.zeros((3, 8), dtype=np.float32)
    rows = sp.csr_matrix((np.array([1.0, 0.1]), np.array([3, 5]), np.array([0, 1, 1, 2])), shape=(3, 8))
    kw = dict(alpha=-3, pre_process_count="linear")
    D = m.posterior_draws(rows, draws=3, sigma=1.0, seed=2, **kw)
    assert np.isnan(D[0]).all() and np.isfinite(D[1:]).all()
    assert (D[1] != 0).all() and np.abs(D[1].astype(np.float64).std()) > 0.3          # an empty row: the prior, variance 1 / 1.1 an axis
    zero = m.posterior_draws(rows, draws=3, sigma=0, **kw)
    assert np.isnan(zero[0]).all() and (_bits(zero[1]) == 0).all() and np.array_equal(_bits(zero[2, 0]), _bits(m.fold_in(rows, **kw)[2]))
    items, scores = m.recommend_thompson_for(rows, 4, sigma=1.0, seed=2, return_scores=True, **kw)
    assert (items[0] == -1).all() and np.isneginf(scores[0]).all() and (items[1:] >= 0).all() and np.isfinite(scores[1:]).all()
    want = np.argsort(-D[1, 0].astype(np.float64), kind="stable")[:4]                 # unit vectors: the score of item j is x_j
    assert np.array_equal(items[1], want) and np.array_equal(_bits(scores[1]), _bits(D[1, 0][want]))
    mean, var = m.score_posterior(rows, np.array([[3, 0, -1], [3, 0, -1], [5, 0, -1]]), **kw)
    assert np.isnan(mean[0, :2]).all() and np.isnan(var[0, :2]).all() and mean[0, 2] == 0 and var[0, 2] == 0
    assert (mean[1] == 0).all() and np.allclose(var[1, :2], 1 / 1.1, rtol=1e-6) and var[1, 2] == 0
    assert var[2, 0] > var[2, 1] > 0                                 # weight -0.3: wider than the prior on its own axis
    items, scores, std = m.recommend_ucb_for(rows, 4, pool=8, c=1.0, return_scores=True, return_std=True, **kw)
    assert (items[0] == -1).all() and np.isneginf(scores[0]).all() and (std[0] == 0).all()
    assert np.array_equal(items[1], [0, 1, 2, 3]) and (items[2] >= 0).all() and (std[1:] > 0).all()
