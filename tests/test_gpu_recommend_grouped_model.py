"""WMF.recommend_shelves, recommend_shelves_for and recommend_capped on small trained models (k = 16, and k = 128 with biases) over
a clustered catalogue: against recommend() under per-row masks with repeated users (items and score bits), the loop over rank(),
recommend_shelves on a model whose users are fold_in(count_rows), and tests/grouped_ref.py's capped_ref on the device's own scores."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import grouped_ref as gref

pytestmark = pytest.mark.gpu

N_USERS, N_ITEMS, N_CLUSTERS, PER = 200, 2000, 40, 50
G = 20
CONFIGS = {"k16": (16, False), "k128b": (128, True)}
USERS = list(range(0, 45)) + [5, 5, -1]


def _counts(seed, n_users=N_USERS):
    """A clustered catalogue: 40 clusters of 50 items; a user draws most counts from two favourite clusters."""
    rng = np.random.default_rng(seed)
    rows, cols, vals = [], [], []
    for u in range(n_users):
        fav = rng.choice(N_CLUSTERS, 2, replace=False)
        for c, k in ((fav[0], 12), (fav[1], 6)):
            rows += [u] * k
            cols += list(c * PER + rng.choice(PER, k, replace=False))
            vals += list(rng.integers(1, 9, k))
        rows += [u] * 3
        cols += list(rng.choice(N_ITEMS, 3, replace=False))
        vals += [1] * 3
    m = sp.coo_matrix((np.asarray(vals, dtype=np.float64), (rows, cols)), shape=(n_users, N_ITEMS)).tocsr()
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


@pytest.fixture(scope="module")
def groups():
    """Two clusters a shelf; every 17th item on no shelf."""
    j = np.arange(N_ITEMS)
    g = np.where(j % 17 == 16, -1, j // (2 * PER))
    g.setflags(write=False)
    return g


def _same(a, b):
    return all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b)) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))


def _by_masks(model, users, groups, n_groups, topn, **kw):
    """The route of recommend()'s docstring: every user once per shelf under the shelf's mask."""
    masks = np.stack([groups == g for g in range(n_groups)])
    rep = np.repeat(np.asarray(users), n_groups)
    items, scores = model.recommend(rep, topn, return_scores=True, allow=masks, allow_idx=np.tile(np.arange(n_groups), len(users)), **kw)
    return items.reshape(len(users), n_groups, topn), scores.reshape(len(users), n_groups, topn)


@pytest.mark.parametrize("topn", (1, 10, 60))
def test_shelves_are_recommend_under_the_shelves_masks(model, counts, groups, topn):
    for kw in ({}, dict(exclude=counts)):
        got = model.recommend_shelves(USERS, groups, topn, return_scores=True, **kw)
        assert got[0].dtype == np.int64 and got[0].shape == (len(USERS), G, topn) and got[1].dtype == np.float32
        assert _same(got, _by_masks(model, USERS, groups, G, topn, **kw)), (topn, list(kw))
        assert np.array_equal(model.recommend_shelves(USERS, groups, topn, **kw), got[0])
    valid = got[0] >= 0
    assert (groups[got[0][valid]] == np.broadcast_to(np.arange(G)[None, :, None], got[0].shape)[valid]).all()
    assert (got[1][~valid] == -np.inf).all() and valid[:, :, 0].all()
    row = model.recommend_shelves(5, groups, topn, exclude=counts)
    assert row.shape == (G, topn) and np.array_equal(row, got[0][5])


def test_shelves_with_an_allow_mask_an_id_list_and_more_shelves_than_used(model, counts, groups):
    rng = np.random.default_rng(21)
    mask = rng.random(N_ITEMS) < 0.3
    want = model.recommend_shelves(USERS, groups, 10, exclude=counts, return_scores=True, allow=mask)
    masks = np.stack([(groups == g) & mask for g in range(G)])
    rep = np.repeat(np.asarray(USERS), G)
    by_rows = model.recommend(rep, 10, exclude=counts, return_scores=True, allow=masks, allow_idx=np.tile(np.arange(G), len(USERS)))
    assert _same(want, [a.reshape(len(USERS), G, 10) for a in by_rows])
    assert _same(model.recommend_shelves(USERS, groups, 10, exclude=counts, return_scores=True, allow=np.flatnonzero(mask)), want)
    two = np.stack([mask, ~mask])
    allow_idx = np.arange(len(USERS)) % 3 - 1
    per_row = model.recommend_shelves(USERS, groups, 10, exclude=counts, return_scores=True, allow=two, allow_idx=allow_idx)
    assert _same([a[allow_idx == 0] for a in per_row], [a[allow_idx == 0] for a in want])
    plain = model.recommend_shelves(USERS, groups, 10, exclude=counts, return_scores=True)
    assert _same([a[allow_idx == -1] for a in per_row], [a[allow_idx == -1] for a in plain])
    wider = model.recommend_shelves(USERS, groups, 10, exclude=counts, return_scores=True, n_groups=64)
    assert wider[0].shape == (len(USERS), 64, 10) and _same([a[:, :G] for a in wider], plain)
    assert (wider[0][:, G:] == -1).all() and (wider[1][:, G:] == -np.inf).all()
    assert (model.recommend_shelves(USERS, groups, 10, allow=[]) == -1).all()
    assert model.recommend_shelves([], groups, 10).shape == (0, G, 10)


def test_shelves_against_the_loop_over_rank(model, counts, groups):
    users = [0, 5, 17, 44]
    items = model.recommend_shelves(users, groups, 10, exclude=counts)
    for b, u in enumerate(users):
        for g in range(G):
            cand = np.setdiff1d(np.flatnonzero(groups == g), counts[u].indices).astype(np.int32)
            best = model.rank(cand, int(u), 10)
            assert len(best) == 10 and (items[b, g] >= 0).all()
            assert np.array_equal(model.predict([u] * 10, items[b, g]), model.predict([u] * 10, best)), (u, g)


def test_a_batch_cut_by_the_workspace_bound_or_the_row_bound_gives_the_same_output(model, counts, groups, monkeypatch):
    from recmodel_amd import _lib, wmf_model
    want = model.recommend_shelves(USERS, groups, 10, exclude=counts, return_scores=True)
    monkeypatch.setattr(wmf_model, "RECOMMEND_BATCH_USERS", 7)
    assert len(USERS) % 7 != 0
    assert _same(model.recommend_shelves(USERS, groups, 10, exclude=counts, return_scores=True), want)
    monkeypatch.setattr(wmf_model, "RECOMMEND_BATCH_USERS", 4096)
    ws = _lib.load().wmf_recommend_grouped_workspace_bytes
    one = int(ws(1, G, 10, 0))
    assert int(ws(2, G, 10, 0)) > one
    for bound in (one, one - 1, 5 * one):                            # one row fills a call (it is never fewer), then a few rows
        monkeypatch.setattr(wmf_model, "CANDIDATES_WS_BYTES", bound)
        assert _same(model.recommend_shelves(USERS, groups, 10, exclude=counts, return_scores=True), want), bound


def test_a_read_only_assignment_is_uploaded_once(model, groups):
    assert not groups.flags.writeable
    model.recommend_shelves([0], groups, 3)
    held = model._groups[id(groups)][1]
    model.recommend_shelves([1], groups, 3)
    assert model._groups[id(groups)][1] is held
    edited = groups.copy()                                           # a writable array is read anew on every call
    a = model.recommend_shelves([0], edited, 3)
    assert (a[0, 0] >= 0).all()
    edited[a[0, 0]] = 1
    b = model.recommend_shelves([0], edited, 3)
    assert id(edited) not in model._groups and not np.isin(a[0, 0], b[0, 0]).any()


def test_shelves_for_is_shelves_on_the_folded_in_rows(model, groups):
    from recmodel_amd import WMF
    B = 9
    rows = _counts(8, B)
    bias = model.bias is True
    dim = model.items.shape[1] - int(bias)
    folded = WMF(num_items=N_ITEMS, num_users=B, dim=dim, gamma=0.1, weighted=True, bias=bias)
    folded.users, folded.items = model.fold_in(rows), model.items
    mask = np.random.default_rng(22).random(N_ITEMS) < 0.4
    for kw in ({}, dict(allow=mask), dict(allow=np.stack([mask, ~mask]), allow_idx=np.arange(B) % 3 - 1)):
        got = model.recommend_shelves_for(rows, groups, 10, return_scores=True, **kw)
        assert got[0].shape == (B, G, 10) and got[0].dtype == np.int64 and got[1].dtype == np.float32
        assert _same(got, folded.recommend_shelves(np.arange(B), groups, 10, exclude=rows, return_scores=True, **kw)), list(kw)
        assert np.array_equal(model.recommend_shelves_for(rows, groups, 10, **kw), got[0])
    free = model.recommend_shelves_for(rows, groups, 10, exclude_history=False, return_scores=True)
    assert _same(free, folded.recommend_shelves(np.arange(B), groups, 10, return_scores=True))
    assert model.recommend_shelves_for(sp.csr_matrix((0, N_ITEMS)), groups, 4).shape == (0, G, 4)


def _device_scores(model):
    """float32 [users, items]: the scores wmf_rank_topn_batch returns for the whole catalogue as the candidate list, in item order
    -- the scan's arithmetic, bit for bit."""
    from recmodel_amd import _lib
    from recmodel_amd.engine import _ptr, _stream
    lib = _lib.load()
    users_t, items_t, f, ld = model._device_factors()
    nu, ni = len(USERS), N_ITEMS
    uu = torch.from_numpy(np.where(np.asarray(USERS) < 0, np.asarray(USERS) + N_USERS, USERS).astype(np.int32)).cuda()
    cand = torch.arange(ni, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(lib.wmf_rank_batch_workspace_bytes(nu, ni)), dtype=torch.uint8, device="cuda")
    pos = torch.empty(nu * ni, dtype=torch.int32, device="cuda")
    sc = torch.empty(nu * ni, dtype=torch.float32, device="cuda")
    _lib.check(lib.wmf_rank_topn_batch(_ptr(users_t), _ptr(items_t), f, ld, int(model.bias is True), _ptr(uu), nu, _ptr(cand), ni, ni, _ptr(pos),
                                       _ptr(sc), _ptr(ws), ws.numel(), _stream()))
    pos, sc = pos.cpu().numpy().reshape(nu, ni), sc.cpu().numpy().reshape(nu, ni)
    D = np.empty_like(sc)
    np.put_along_axis(D, pos.astype(np.int64), sc, axis=1)
    return D


def test_capped_lists(model, counts, groups):
    D = _device_scores(model)
    for topn, per_group in ((10, 1), (10, 2), (10, 3), (25, 1), (128, 4), (5, 10)):
        items, scores = model.recommend_capped(USERS, groups, topn, per_group, exclude=counts, return_scores=True)
        assert items.shape == (len(USERS), topn) and items.dtype == np.int64 and scores.dtype == np.float32
        for b, u in enumerate(USERS):
            want = gref.capped_ref(D[b].astype(np.float64), counts[u].indices, groups, G, topn, per_group)
            assert np.array_equal(items[b, :len(want)], want) and (items[b, len(want):] == -1).all(), (topn, per_group, b)
            assert np.array_equal(scores[b, :len(want)].view(np.int32), D[b, want].view(np.int32)) and (scores[b, len(want):] == -np.inf).all()
            assert np.bincount(groups[want], minlength=G).max() <= per_group
        assert np.array_equal(model.recommend_capped(USERS, groups, topn, per_group, exclude=counts), items)
    one = model.recommend_capped(USERS, groups, 10, 1, exclude=counts)
    assert all(len(set(groups[r[r >= 0]])) == (r >= 0).sum() for r in one)      # per_group = 1: at most one item of a shelf
    assert (one[:, :10] >= 0).all()                                              # (twenty shelves: ten are found)
    row = model.recommend_capped(5, groups, 10, 2, exclude=counts)
    assert row.shape == (10,) and np.array_equal(row, model.recommend_capped(USERS, groups, 10, 2, exclude=counts)[5])


def test_a_loose_cap_on_one_shelf_is_recommend(model, counts):
    everything = np.zeros(N_ITEMS, dtype=np.int64)
    for topn, per_group in ((10, 10), (10, 500), (128, 128)):
        assert _same(model.recommend_capped(USERS, everything, topn, per_group, exclude=counts, return_scores=True),
                     model.recommend(USERS, topn, exclude=counts, return_scores=True)), (topn, per_group)
