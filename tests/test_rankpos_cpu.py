"""What the exact full-catalogue ranks promise without a GPU: the host reference of the GPU tests (tests/rankpos_ref.py) against
the reference of the top-n it is the dual of (tests/recommend_ref.py), the metric formulas against hand-computed numbers,
RecModel.eval_ranking on a model that only has predict() and rank(), and the argument checks of wmf_rank_positions, which happen
before anything touches the device."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import rankpos_ref as pref
import recommend_ref as rref
from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build()
    from recmodel_amd import _lib
    return _lib.load()


def _header_constants():
    text = open(os.path.join(ROOT, "include", "wmf_hip.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define\s+(WMF_(?:RANKPOS|RECOMMEND)_[A-Z_]+)\s+\(?(-?\d+)\)?", text)}


# ------------------------------------------------------------------------------------------------------- the host reference
def test_rank_below_k_is_membership_in_the_top_k():
    """Tied integer scores: for every k, rank < k exactly when the item is among recommend_ref's first k."""
    rng = np.random.default_rng(7)
    n_items = 60
    for trial in range(30):
        scores = rng.integers(-3, 4, n_items).astype(np.int64 if trial % 2 else np.float64)
        seen = rng.choice(n_items, int(rng.integers(0, 40)), replace=True)
        if trial == 0:
            seen = np.arange(n_items)                               # everything seen
        if trial == 1:
            seen = np.arange(0)
        ranks = pref.rank_positions_ref(scores, seen, np.arange(n_items))
        assert np.array_equal(ranks == pref.SEEN, np.isin(np.arange(n_items), seen))
        unseen = ranks[ranks >= 0]
        assert np.array_equal(np.sort(unseen), np.arange(len(unseen)))                # a permutation of the places
        for k in range(1, n_items + 2):
            top = rref.recommend_ref(scores, seen, k)
            assert np.array_equal(np.isin(np.arange(n_items), top), (ranks >= 0) & (ranks < k)), (trial, k)
            assert np.array_equal(ranks[top], np.arange(len(top))), (trial, k)


def test_rank_positions_ref_ties_and_duplicates():
    scores = np.array([5, 7, 7, 1, 7, 5], dtype=np.int64)
    assert pref.rank_positions_ref(scores, [], [1, 2, 4, 0, 5, 3]).tolist() == [0, 1, 2, 3, 4, 5]
    assert pref.rank_positions_ref(scores, [2, 2, 1], [4, 4, 2, 3, 0]).tolist() == [0, 0, pref.SEEN, 3, 1]
    assert pref.rank_positions_ref(scores, [0], []).tolist() == []


# -------------------------------------------------------------------------------------------------------------- the metrics
def _hand_case():
    """Four users: no targets; a hit at place 0 and a seen target; a duplicated target at place 2 and one at place 5; one
    target at place 1, fewer than k."""
    return [[], [0, pref.SEEN], [2, 2, 5], [1]]


def _hand_numbers():
    l3, l7 = 1.0 / math.log2(3.0), 1.0 / math.log2(7.0)
    ideal_c = 1.0 + l3                                              # user C has two distinct unseen targets
    return {
        "Recall@1": 1 / 6, "Precision@1": 1 / 3, "ARHR@1": 1 / 6, "NDCG@1": (1.0 + 0.0 + 0.0) / 3,
        "Recall@3": 4 / 6, "Precision@3": 4 / 9, "ARHR@3": (1 + 1 / 3 + 1 / 3 + 1 / 2) / 6, "NDCG@3": (1.0 + (0.5 + 0.5) / ideal_c + l3) / 3,
        "Recall@10": 5 / 6, "Precision@10": 5 / 30, "ARHR@10": (1 + 1 / 3 + 1 / 3 + 1 / 6 + 1 / 2) / 6,
        "NDCG@10": (1.0 + (0.5 + 0.5 + l7) / ideal_c + l3) / 3,
    }


def test_metric_formulas_against_a_hand_computed_case():
    from recmodel_amd.base_model import ranking_metrics
    rows, want = _hand_case(), _hand_numbers()
    topn = np.array([1, 3, 10])
    got_ref = pref.ranking_metrics_ref(rows, topn)
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    got = ranking_metrics(indptr, np.concatenate([np.asarray(r, dtype=np.int64) for r in rows]), topn)
    assert sorted(got_ref) == sorted(got) == sorted(want)
    for name, value in want.items():
        assert got_ref[name] == pytest.approx(value, rel=1e-14, abs=0), name
        assert got[name] == pytest.approx(value, rel=1e-14, abs=0), name
        assert isinstance(got[name], float)
    empty = ranking_metrics(np.zeros(3, dtype=np.int64), np.zeros(0, dtype=np.int64), np.array([5]))
    assert all(math.isnan(v) for v in empty.values()) and all(math.isnan(v) for v in pref.ranking_metrics_ref([[], []], [5]).values())


# --------------------------------------------------------------------------------------------- eval_ranking, the fallback path
def _numpy_model(S):
    from recmodel_amd import RecModel

    class Dense(RecModel):
        """predict() and rank() on a dense score matrix, nothing else; equal scores keep candidate order."""

        def predict(self, users, items):
            return S[np.asarray(users), np.asarray(items)]

        def rank(self, items, users, topn=None):
            items = np.asarray(items)
            order = np.argsort(-S[users, items], kind="stable")
            return items[order[:topn]]
    return Dense()


def _ref_metrics(S, test, train, users, topn):
    rows = []
    for u in users:
        seen = train[u].indices if train is not None else []
        rows.append(pref.rank_positions_ref(S[u], seen, np.unique(test[u].indices)))
    return pref.ranking_metrics_ref(rows, topn)


def test_eval_ranking_through_rank_equals_the_reference_and_leaves_its_inputs_alone():
    rng = np.random.default_rng(3)
    n_users, n_items = 9, 31
    S = rng.integers(-4, 5, (n_users, n_items)).astype(np.float64)                   # ties
    model = _numpy_model(S)
    train = sp.random(n_users, n_items, density=0.3, format="csr", random_state=1, dtype=np.float32)
    test = sp.random(n_users, n_items, density=0.15, format="lil", random_state=2, dtype=np.float32)
    test[4, :] = 0.0                                                # a user without targets
    test[2, train[2].indices[:2]] = 1.0                             # seen targets
    test = sp.csr_matrix(test)
    test.eliminate_zeros()
    test.data[::4] = 0.0                                            # stored zeros are targets
    assert test[4].nnz == 0 and test.nnz > 10
    # unsorted, duplicated COO input of the same matrix: every entry split in two halves, in reverse order
    coo = test.tocoo()
    messy = sp.coo_matrix((np.concatenate([coo.data, coo.data])[::-1] / 2, (np.concatenate([coo.row, coo.row])[::-1],
                                                                           np.concatenate([coo.col, coo.col])[::-1])), shape=test.shape)
    keep = [(m.data.copy(), m.indices.copy(), m.indptr.copy()) for m in (test, train)]
    topn = np.array([1, 5, 10, 40])
    everyone = np.flatnonzero(np.diff(test.indptr))
    want = _ref_metrics(S, test, train, everyone, topn)
    same = lambda a, b: sorted(a) == sorted(b) and all(a[k] == pytest.approx(b[k], rel=1e-12, abs=0) for k in b)  # noqa: E731  (float64 sums in two orders)
    for mat, seen in ((test, train), (messy, train), (messy, train.tocoo()), (test.tolil(), train.tocsc())):
        got = model.eval_ranking(mat, train_mat=seen, topn=topn)
        assert same(got, want), (got, want)
    assert 0 < want["Recall@5"] < want["Recall@40"] < 1.0           # (the seen targets are misses at every k)
    assert same(model.eval_ranking(test, topn=topn), _ref_metrics(S, test, None, everyone, topn))
    sub = [0, -1, 4, 2]
    assert same(model.eval_ranking(test, train, topn, users=sub), _ref_metrics(S, test, train, [0, n_users - 1, 4, 2], topn))
    for (data, indices, indptr), m in zip(keep, (test, train)):
        assert np.array_equal(m.data, data) and np.array_equal(m.indices, indices) and np.array_equal(m.indptr, indptr)
    with pytest.raises(ValueError):
        model.eval_ranking(test, train, topn=[10])
    with pytest.raises(ValueError):
        model.eval_ranking(test.toarray(), train, topn=topn)
    with pytest.raises(ValueError):
        model.eval_ranking(test, train.T.tocsr(), topn=topn)
    with pytest.raises(IndexError):
        model.eval_ranking(test, train, topn=topn, users=[n_users])


def test_rank_positions_checks_its_arguments_before_the_gpu():
    import torch
    from recmodel_amd import WMF, _lib
    m = WMF(num_items=12, num_users=5, dim=3, gamma=0.1, weighted=True)
    m.users = np.random.default_rng(0).random((5, 3)).astype(np.float32)
    test = sp.random(5, 12, density=0.3, format="csr", random_state=0)
    with pytest.raises(ValueError):
        m.rank_positions(test.toarray())
    with pytest.raises(ValueError):
        m.rank_positions(sp.csr_matrix((5, 11)))
    with pytest.raises(ValueError):
        m.rank_positions(test, exclude=test.T.tocsr(), users=[99])  # the shapes are looked at first
    with pytest.raises(IndexError):
        m.rank_positions(test, exclude=test, users=[0, 5])
    with pytest.raises(IndexError):
        m.rank_positions(test, users=-6)
    with pytest.raises(ValueError):
        m.eval_ranking(test, test, topn=[10])
    if not torch.cuda.is_available():
        with pytest.raises(_lib.WmfLibraryError):
            m.rank_positions(test, exclude=test, users=[0, -5])
        with pytest.raises(_lib.WmfLibraryError):
            m.eval_ranking(test, test, topn=np.array([10]))


# ------------------------------------------------------------------------------------------------------------------ the ABI
def test_rank_positions_symbols_and_constants(lib):
    from recmodel_amd import _lib, wmf_model
    K = _header_constants()
    for name in ("wmf_rank_positions", "wmf_rank_positions_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert K["WMF_RANKPOS_MAX_TARGETS"] >= 16 and K["WMF_RANKPOS_MAX_TARGETS"] % 16 == 0
    assert K["WMF_RANKPOS_MAX_TARGETS"] == wmf_model.RANKPOS_MAX_TARGETS
    assert (K["WMF_RANKPOS_SEEN"], K["WMF_RANKPOS_BEYOND"]) == (pref.SEEN, pref.BEYOND) == (-1, -2)
    from recmodel_amd import base_model
    assert base_model.RANKPOS_SEEN == pref.SEEN
    size = lambda rows, targets, slices: int(lib.wmf_rank_positions_workspace_bytes(rows, targets, slices))  # noqa: E731
    assert size(100, 5, 0) == K["WMF_RANKPOS_WS_BASE"] + 100 * K["WMF_RANKPOS_WS_PER_ROW"]
    for rows in (1, 17, 4096):
        assert len({size(rows, t, s) for t in (0, 1, 10 ** 6) for s in (0, 1, 64, K["WMF_RECOMMEND_MAX_SLICES"])}) == 1
        assert size(rows, 1, 0) < size(rows + 1, 1, 0)


def _call(lib, users=16, items=16, f=5, ld=8, user_idx=16, n_rows=3, n_items=20, seen_indptr=0, seen_indices=0, target_indptr=16,
          target_indices=16, n_slices=0, out_rank=16, ws=16, ws_bytes=None):
    vp = lambda a: ctypes.c_void_p(a) if a else None  # noqa: E731
    if ws_bytes is None:
        ws_bytes = int(lib.wmf_rank_positions_workspace_bytes(max(n_rows, 1), 0, max(n_slices, 0)))
    return lib.wmf_rank_positions(vp(users), vp(items), f, ld, 1, vp(user_idx), n_rows, n_items, vp(seen_indptr), vp(seen_indices),
                                  vp(target_indptr), vp(target_indices), n_slices, vp(out_rank), None, vp(ws), ws_bytes, None)


def test_rank_positions_argument_validation_without_gpu(lib):
    """Every refusal comes before the first HIP call: the pointers below are not device memory."""
    from recmodel_amd import _lib
    K = _header_constants()
    for bad in (dict(n_rows=0), dict(n_items=0), dict(n_items=2 ** 31), dict(n_slices=-1), dict(n_slices=K["WMF_RECOMMEND_MAX_SLICES"] + 1),
                dict(ld=7), dict(ld=4), dict(f=0), dict(ld=276, f=273), dict(users=0), dict(items=0), dict(user_idx=0),
                dict(target_indptr=0), dict(target_indices=0), dict(out_rank=0), dict(ws=0), dict(seen_indptr=16), dict(seen_indices=16)):
        assert _call(lib, **bad) == _lib.WMF_EINVAL, bad
        assert lib.wmf_last_error(), bad
        with pytest.raises(ValueError):
            _lib.check(_call(lib, **bad))
    need = int(lib.wmf_rank_positions_workspace_bytes(3, 0, 2))
    assert _call(lib, n_slices=2, ws_bytes=need - 1) == _lib.WMF_EINVAL
    assert b"workspace" in lib.wmf_last_error()
