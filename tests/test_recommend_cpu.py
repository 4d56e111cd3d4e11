"""What the full-catalogue recommendation promises without a GPU: the host reference of the GPU tests (tests/recommend_ref.py)
against the CPU reference implementation's rank(), the argument checks of wmf_recommend_topn and WMF.recommend, which happen
before anything touches the device, and utils.test_coverage on a model that only has rank()."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import recommend_ref as rref
import serving_ref as ref
from conftest import ROOT

WIDTHS = (1, 4, 5, 16, 63, 64, 65, 100, 128, 129, 144, 192, 193, 256, 257, 260)      # those of tests/test_gpu_serving.py
N_USERS, N_ITEMS = 40, 300


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build()
    from recmodel_amd import _lib
    return _lib.load()


def _header_constants():
    text = open(os.path.join(ROOT, "include", "wmf_hip.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define\s+(WMF_RECOMMEND_[A-Z_]+)\s+(\d+)", text)}


# ------------------------------------------------------------------------------------------------------- the host reference
@pytest.mark.parametrize("f", WIDTHS)
def test_recommend_ref_is_the_reference_rank_of_the_unseen_items(f):
    from oracle import wmf_oracle as orc
    U = ref.rounded_factors(N_USERS, f, 10 * f + 1).astype(np.float64)
    I = ref.rounded_factors(N_ITEMS, f, 10 * f + 2).astype(np.float64)
    rng = np.random.default_rng(f)
    everything = np.arange(N_ITEMS)
    for bias in ((False, True) if f >= 2 else (False,)):
        for u in range(N_USERS):
            scores = orc.predict(U, I, [u], everything, bias)
            # the reference's tie order is whatever argsort leaves: the comparison needs distinct scores
            assert len(np.unique(scores)) == N_ITEMS, (f, bias, u)
            seen = rng.choice(N_ITEMS, int(rng.integers(0, 60)), replace=False)
            want = orc.rank(U, I, np.delete(everything, seen), u, topn=10, bias=bias)
            got = rref.recommend_ref(scores, seen, 10)
            assert np.array_equal(got, want), (f, bias, u)
            assert not np.isin(got, seen).any()


def test_recommend_ref_ties_padding_and_duplicates():
    scores = np.array([5, 7, 7, 1, 7, 5], dtype=np.int64)
    assert rref.recommend_ref(scores, [], 4).tolist() == [1, 2, 4, 0]
    assert rref.recommend_ref(scores, [2, 2, 1], 4).tolist() == [4, 0, 5, 3]         # fewer eligible than topn: all of them
    assert rref.recommend_ref(scores, np.arange(6), 3).tolist() == []


# ------------------------------------------------------------------------------------------------------------------ the ABI
def _call(lib, users=16, items=16, f=5, ld=8, user_idx=16, n_users=3, n_items=20, topn=10, n_slices=0, out_items=16, ws=16,
          ws_bytes=None):
    vp = lambda a: ctypes.c_void_p(a) if a else None  # noqa: E731
    if ws_bytes is None:
        ws_bytes = int(lib.wmf_recommend_workspace_bytes(max(n_users, 1), min(max(topn, 1), 128), max(n_slices, 0)))
    return lib.wmf_recommend_topn(vp(users), vp(items), f, ld, 1, vp(user_idx), n_users, n_items, None, None, topn, n_slices,
                                  vp(out_items), None, None, vp(ws), ws_bytes, None)


def test_recommend_argument_validation_without_gpu(lib):
    """Every refusal comes before the first HIP call: the pointers below are not device memory."""
    from recmodel_amd import _lib
    K = _header_constants()
    assert K["WMF_RECOMMEND_MAX_TOPN"] == 128
    for bad in (dict(topn=0), dict(topn=129), dict(n_users=0), dict(n_items=0), dict(n_items=2 ** 31), dict(n_slices=-1),
                dict(n_slices=K["WMF_RECOMMEND_MAX_SLICES"] + 1), dict(ld=7), dict(ld=4), dict(users=0), dict(out_items=0),
                dict(items=0), dict(user_idx=0), dict(ws=0)):
        assert _call(lib, **bad) == _lib.WMF_EINVAL, bad
        assert lib.wmf_last_error(), bad
        with pytest.raises(ValueError):
            _lib.check(_call(lib, **bad))
    need = int(lib.wmf_recommend_workspace_bytes(3, 10, 2))
    assert _call(lib, n_slices=2, ws_bytes=need - 1) == _lib.WMF_EINVAL
    assert b"workspace" in lib.wmf_last_error()


def test_recommend_workspace_bytes(lib):
    K = _header_constants()
    cap, c0, c1 = K["WMF_RECOMMEND_AUTO_SLICES"], K["WMF_RECOMMEND_WS_BASE"], K["WMF_RECOMMEND_WS_PER_KEY"]
    users, topns, slices = (1, 2, 17, 4096, 10 ** 6), (1, 2, 10, 127, 128), (1, 2, 3, 64, 65, K["WMF_RECOMMEND_MAX_SLICES"])
    size = lambda u, t, s: int(lib.wmf_recommend_workspace_bytes(u, t, s))  # noqa: E731
    for u in users:
        for t in topns:
            for s in slices + (0,):
                got = size(u, t, s)
                assert 0 < got <= c0 + c1 * u * t * max(s, cap), (u, t, s, got)
            assert size(u, t, 0) == size(u, t, cap)                                 # sized for whatever the library may choose
            assert all(size(u, t, a) <= size(u, t, b) for a, b in zip(slices, slices[1:]))
        for s in slices + (0,):
            assert all(size(u, a, s) <= size(u, b, s) for a, b in zip(topns, topns[1:]))
    for t in topns:
        for s in slices + (0,):
            assert all(size(a, t, s) <= size(b, t, s) for a, b in zip(users, users[1:]))


# --------------------------------------------------------------------------------------------------------- the class surface
def _model():
    from recmodel_amd import WMF
    m = WMF(num_items=12, num_users=5, dim=3, gamma=0.1, weighted=True)
    m.users = np.random.default_rng(0).random((5, 3)).astype(np.float32)
    return m


def test_recommend_checks_its_arguments_before_the_gpu():
    import torch
    from recmodel_amd import _lib
    m = _model()
    train = sp.random(5, 12, density=0.3, format="csr", random_state=0)
    with pytest.raises(ValueError):
        m.recommend([0, 1], exclude=sp.csr_matrix((5, 11)))
    with pytest.raises(ValueError):
        m.recommend([99], topn=0, exclude=train.T.tocsr())         # the shape is looked at first
    with pytest.raises(IndexError):
        m.recommend([0, 5], exclude=train)
    with pytest.raises(IndexError):
        m.recommend(-6, topn=0)                                     # ... the users second
    with pytest.raises(ValueError):
        m.recommend([0, -5], topn=0, exclude=train)
    if not torch.cuda.is_available():
        with pytest.raises(_lib.WmfLibraryError):
            m.recommend([0, -5], topn=3, exclude=train)
        with pytest.raises(_lib.WmfLibraryError):
            m.recommend(2, topn=300)


class _RankOnly:
    """A model with nothing but rank(): dense NumPy scores."""

    def __init__(self, S):
        self.S = S

    def rank(self, items, users, topn=None):
        items = np.asarray(items)
        order = np.argsort(-self.S[users, items], kind="stable")
        return items[order[:topn]]


def test_coverage_of_a_model_that_only_ranks():
    """More items than users: the reference's Train.shape[0] counters would not hold the item ids."""
    import recmodel_amd
    from recmodel_amd import utils
    assert recmodel_amd.test_coverage is utils.test_coverage and utils.test_coverage.__test__ is False
    rng = np.random.default_rng(1)
    n_users, n_items, topn = 7, 23, 4
    model = _RankOnly(rng.permuted(np.arange(n_users * n_items)).reshape(n_users, n_items).astype(np.float64))
    train = sp.random(n_users, n_items, density=0.4, format="csr", random_state=2)
    train[3, :] = 1.0                                               # a user who has seen everything
    train = sp.csr_matrix(train)
    want = np.zeros(n_items, dtype=np.int32)
    for user in range(n_users):
        unseen = np.delete(np.arange(n_items, dtype=np.int32), train.indices[train.indptr[user]:train.indptr[user + 1]])
        want[model.rank(users=user, items=unseen, topn=topn)[:topn]] += 1
    got = utils.test_coverage(model, train, topn)
    assert got.dtype == np.int32 and got.shape == (n_items,) and np.array_equal(got, want)
    assert want.sum() == sum(min(topn, n_items - train[u].nnz) for u in range(n_users)) and want[n_users:].sum() > 0
