"""WMF.recommend_diverse, recommend_diverse_for, rerank_mmr and intra_list_similarity on small trained models (k = 16, and k = 128
with biases) over a clustered catalogue: against recommend / candidates / fold_in, which they are built on, and against
tests/mmr_ref.py step by step (the condition of tests/test_gpu_mmr.py, through the public methods)."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import mmr_ref as mref

pytestmark = pytest.mark.gpu

N_USERS, N_ITEMS, N_CLUSTERS = 300, 400, 16
CONFIGS = {"k16": (16, False), "k128b": (128, True)}


def _counts(seed):
    """A clustered catalogue: 16 groups of 25 items; a user draws most counts from two favourite groups, so a plain top-10 is ten
    items of one group and MMR has near-duplicates to thin out."""
    rng = np.random.default_rng(seed)
    rows, cols, vals = [], [], []
    for u in range(N_USERS):
        fav = rng.choice(N_CLUSTERS, 2, replace=False)
        for g, k in ((fav[0], 12), (fav[1], 6)):
            items = g * 25 + rng.choice(25, k, replace=False)
            rows += [u] * k
            cols += list(items)
            vals += list(rng.integers(1, 9, k))
        extra = rng.choice(N_ITEMS, 3, replace=False)
        rows += [u] * 3
        cols += list(extra)
        vals += [1] * 3
    m = sp.coo_matrix((np.asarray(vals, dtype=np.float64), (rows, cols)), shape=(N_USERS, N_ITEMS)).tocsr()
    m.sum_duplicates()
    return m


@pytest.fixture(scope="module")
def counts():
    return _counts(4)


@pytest.fixture(scope="module", params=list(CONFIGS))
def model(request, counts):
    from recmodel_amd import WMF
    dim, bias = CONFIGS[request.param]
    m = WMF(num_items=N_ITEMS, num_users=N_USERS, dim=dim, gamma=0.1, weighted=True, bias=bias)
    m.train(utility_mat=counts, iterations=3, eval_mat=counts, count_mat=counts)
    return m


USERS = list(range(0, 60)) + [5, 5, -1]


def _bits_equal(a, b):
    return all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b)) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))


def test_lambda_one_is_recommend(model, counts):
    for kw in ({}, dict(exclude=counts), dict(exclude=counts, allow=np.arange(0, N_ITEMS, 2))):
        for topn, pool in ((10, None), (1, 1), (128, 128), (7, 300)):
            got = model.recommend_diverse(USERS, topn, pool=pool, lam=1.0, return_scores=True, **kw)
            assert _bits_equal(got, model.recommend(USERS, topn, return_scores=True, **kw)), (list(kw), topn, pool)
    row = model.recommend_diverse(5, 10, lam=1.0)
    assert row.shape == (10,) and np.array_equal(row, model.recommend(5, 10))


@pytest.mark.parametrize("metric", ("cosine", "dot"))
def test_every_step_is_optimal_within_the_bound_and_the_lists_are_less_alike(model, counts, metric):
    bias, cosine = model.bias is True, metric == "cosine"
    topn, pool, lam = 10, 100, 0.5
    pool_items, pool_scores = model.candidates(USERS, pool, exclude=counts, return_scores=True)
    items, scores = model.recommend_diverse(USERS, topn, pool=pool, lam=lam, metric=metric, exclude=counts, return_scores=True)
    assert items.dtype == np.int64 and items.shape == (len(USERS), topn) and scores.dtype == np.float32
    F = np.asarray(model.items, dtype=np.float32)
    worst, ref_lists = 0.0, []
    for b in range(len(USERS)):
        c = int((pool_items[b] >= 0).sum())
        assert c == pool
        assert set(items[b]) <= set(pool_items[b]) and len(set(items[b])) == topn     # a subset of the pool, nothing twice
        pos = np.array([int(np.flatnonzero(pool_items[b] == i)[0]) for i in items[b]])
        assert np.array_equal(scores[b].view(np.int32), pool_scores[b, pos].view(np.int32))
        for t, (short, e) in enumerate(mref.step_shortfalls(F, bias, pool_items[b], pool_scores[b], pos, lam, cosine)):
            print(f"{metric} row {b} step {t}: shortfall {short:.3e}, E {e:.3e}")
            assert short <= 2 * e, (b, t, short, e)
            worst = max(worst, short / e if e > 0 else 0.0)
        picks, _ = mref.mmr_greedy(pool_scores[b], mref.RowSims(F, bias, pool_items[b], cosine, "f64").column, lam, topn, np.float64)
        ref_lists.append(pool_items[b, picks])
    print(f"largest shortfall: {worst:.3f} E")
    # the same lists through rerank_mmr: host arrays, device tensors, an explicit count
    assert _bits_equal((items, scores), model.rerank_mmr(pool_items, pool_scores, topn, lam, metric, return_scores=True))
    dev = model.rerank_mmr(torch.from_numpy(pool_items.astype(np.int32)).cuda(), torch.from_numpy(pool_scores).cuda(), topn, lam, metric,
                           pool_count=torch.full((len(USERS),), pool, dtype=torch.int32, device="cuda"), return_scores=True)
    assert _bits_equal((items, scores), dev)
    short = model.rerank_mmr(pool_items, pool_scores, topn, lam, metric, pool_count=np.full(len(USERS), 4))
    assert (short[:, 4:] == -1).all() and all(set(short[b, :4]) == set(pool_items[b, :4]) for b in range(len(USERS)))
    # intra-list similarity: the device's figures against float64 within the bound, and the diversified lists are less alike
    plain = model.recommend(USERS, topn, exclude=counts)
    mean_div, top_div = model.intra_list_similarity(items, metric)
    mean_plain, _ = model.intra_list_similarity(plain, metric)
    for b in (0, 17, len(USERS) - 1):
        m64, bm, t64, bt = mref.ils_bounds(F, bias, items[b], cosine)
        assert abs(float(mean_div[b]) - m64) <= bm and abs(float(top_div[b]) - t64) <= bt
    ref_div = np.mean([mref.ils_bounds(F, bias, row, cosine)[0] for row in ref_lists])
    ref_plain = np.mean([mref.ils_bounds(F, bias, row, cosine)[0] for row in plain])
    print(f"{metric}: mean intra-list similarity {float(mean_plain.mean()):.4f} plain, {float(mean_div.mean()):.4f} diversified; "
          f"reference {ref_plain:.4f} -> {ref_div:.4f}")
    assert ref_div < ref_plain, "the dataset must show a strict drop in the reference"
    assert float(mean_div.astype(np.float64).mean()) <= float(mean_plain.astype(np.float64).mean())
    one_mean, one_top = model.intra_list_similarity(items[3], metric)
    assert one_mean == mean_div[3] and one_top == top_div[3]
    padded = np.concatenate([items[:2, :3], np.full((2, 2), -1)], axis=1)               # -1 ends a list
    pm, pt = model.intra_list_similarity(padded, metric)
    sm, st = model.intra_list_similarity(items[:2, :3], metric)
    assert np.array_equal(pm, sm) and np.array_equal(pt, st)
    em, et = model.intra_list_similarity(np.array([[7, -1, -1], [-1, -1, -1]]), metric)
    assert (em == 0).all() and (et == -np.inf).all()


def test_filters_are_honoured(model, counts):
    users = np.arange(40)
    got = model.recommend_diverse(users, 10, pool=60, lam=0.4, exclude=counts)
    for b, u in enumerate(users):
        assert not set(got[b]) & set(counts[u].indices), "a seen item was returned"
    mask = np.random.default_rng(2).random(N_ITEMS) < 0.3
    for kw in (dict(allow=mask), dict(allow=np.flatnonzero(mask))):
        got = model.recommend_diverse(users, 10, pool=60, lam=0.4, exclude=counts, **kw)
        assert mask[got[got >= 0]].all() and (got >= 0).all()
    G = np.stack([mask, ~mask, np.zeros(N_ITEMS, dtype=bool)])
    G[2, [3, 9, 11]] = True
    idx = np.arange(40) % 4 - 1                                     # -1: unrestricted
    got = model.recommend_diverse(users, 10, pool=60, lam=0.4, allow=G, allow_idx=idx)
    for b in range(40):
        if idx[b] >= 0:
            assert G[idx[b]][got[b][got[b] >= 0]].all()
        if idx[b] == 2:                                             # three eligible items: three picks, then padding
            assert set(got[b, :3]) == {3, 9, 11} and (got[b, 3:] == -1).all()
    seen_all = sp.csr_matrix(np.ones((N_USERS, N_ITEMS), dtype=np.float32))
    assert (model.recommend_diverse([1, 2], 5, exclude=seen_all) == -1).all()
    assert model.recommend_diverse([], 5).shape == (0, 5)


def test_histories_agree_with_a_model_of_their_fold_in(model, counts):
    from recmodel_amd import WMF
    hist = counts[100:140]
    dim, bias = model.dim, model.bias
    other = WMF(num_items=N_ITEMS, num_users=hist.shape[0], dim=dim, gamma=model.gamma, weighted=True, bias=bias)
    other.items = model.items
    other.users = model.fold_in(hist)
    for lam, metric in ((0.6, "cosine"), (0.2, "dot"), (1.0, "cosine")):
        a = model.recommend_diverse_for(hist, 10, pool=80, lam=lam, metric=metric, return_scores=True)
        b = other.recommend_diverse(np.arange(hist.shape[0]), 10, pool=80, lam=lam, metric=metric, exclude=hist, return_scores=True)
        assert _bits_equal(a, b), (lam, metric)
    a = model.recommend_diverse_for(hist, 5, exclude_history=False, lam=0.5)
    assert np.array_equal(a, other.recommend_diverse(np.arange(hist.shape[0]), 5, lam=0.5))


def test_batches_of_one_three_and_more_than_a_window(model, counts, monkeypatch):
    from recmodel_amd import wmf_model
    users = np.arange(50)
    whole = model.recommend_diverse(users, 10, pool=50, lam=0.5, exclude=counts, return_scores=True)
    for n in (1, 3):
        assert _bits_equal(model.recommend_diverse(users[:n], 10, pool=50, lam=0.5, exclude=counts, return_scores=True), [a[:n] for a in whole])
    monkeypatch.setattr(wmf_model, "RECOMMEND_BATCH_USERS", 16)     # 50 rows: four windows, the last one of two rows
    assert _bits_equal(model.recommend_diverse(users, 10, pool=50, lam=0.5, exclude=counts, return_scores=True), whole)
    hist = counts[:50]
    for_whole = model.recommend_diverse_for(hist, 10, pool=50, lam=0.5, return_scores=True)
    monkeypatch.setattr(wmf_model, "RECOMMEND_BATCH_USERS", 4096)
    assert _bits_equal(model.recommend_diverse_for(hist, 10, pool=50, lam=0.5, return_scores=True), for_whole)
