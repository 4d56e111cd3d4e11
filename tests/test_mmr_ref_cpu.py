"""The diversified top-n without a GPU: tests/mmr_ref.py against a brute-force restatement, its edge rules, the argument checks of
the Python methods and every refusal of the three C entry points (they come before any HIP call, so the shipped library answers
them here), the routing formula and the ABI table."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import mmr_ref as mref
import serving_ref as ref


# ------------------------------------------------------------------------------------------------------- the reference itself
def _brute(r, M, lam, topn, dtype):
    """Greedy MMR with every maximum recomputed from scratch at every step: M[j, p] = sim(j, p)."""
    r = np.asarray(r, dtype=dtype)
    lam_t = dtype(np.float32(lam))
    mu = dtype(1) - lam_t
    picks, values = [], []
    for t in range(min(topn, len(r))):
        best, best_v = None, None
        for j in range(len(r)):
            if j in picks:
                continue
            v = lam_t * r[j]
            if picks:
                v = v - mu * max(dtype(M[j, p]) for p in picks)
            if best is None or v > best_v:
                best, best_v = j, v
        picks.append(best)
        values.append(best_v)
    return np.array(picks, dtype=np.int64), np.array(values, dtype=dtype)


def _pool(n_items, c, seed, duplicate=True):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, n_items, c)
    if duplicate and c >= 3:
        ids[c // 2] = ids[0]                                        # an id listed twice is two candidates
    return ids


@pytest.mark.parametrize("f,bias", [(1, 0), (5, 1), (16, 0), (33, 1)])
@pytest.mark.parametrize("cosine", (False, True))
def test_reference_against_brute_force(f, bias, cosine):
    for seed, c, topn in ((1, 1, 3), (2, 2, 2), (3, 17, 17), (4, 40, 9)):
        ids = _pool(50, c, seed)
        rng = np.random.default_rng(seed)
        # exact inputs: the float32 form, the float64 form (and, for the dot, the integer form) are one sequence
        F = mref.pow4_items(50, f, bias, seed) if cosine else mref.exact_items(50, f, seed)
        r = rng.integers(-5, 6, c).astype(np.float32)
        for lam in mref.LAMBDAS:
            s32, s64 = mref.RowSims(F, bias, ids, cosine, "f32"), mref.RowSims(F, bias, ids, cosine, "f64")
            p32, v32 = mref.mmr_greedy(r, s32.column, lam, topn, np.float32)
            p64, v64 = mref.mmr_greedy(r, s64.column, lam, topn, np.float64)
            pb, vb = _brute(r, s32.matrix(), lam, topn, np.float32)
            assert np.array_equal(p32, pb) and np.array_equal(v32, vb), (f, bias, cosine, lam, c)
            assert np.array_equal(p32, p64) and np.array_equal(v32.astype(np.float64), v64), "exact inputs: every float32 operation is exact"
            assert len(set(p32)) == len(p32) == min(topn, c)
            if not cosine:
                pi, vi = mref.mmr_greedy_int(r, mref.RowSims(F, bias, ids, False, "int").column, int(4 * lam), topn)
                assert np.array_equal(pi, p32) and np.array_equal(vi, 4 * v64)
        # Gaussian inputs: the float64 form against the brute force in float64
        G = ref.rounded_factors(50, f, seed + 10)
        rg = rng.standard_normal(c).astype(np.float32)
        sg = mref.RowSims(G, bias, ids, cosine, "f64")
        for lam in (0.0, 0.3, 0.7, 1.0):
            pg, vg = mref.mmr_greedy(rg, sg.column, lam, topn, np.float64)
            pb, vb = _brute(rg, sg.matrix(), lam, topn, np.float64)
            assert np.array_equal(pg, pb) and np.allclose(vg, vb, rtol=0, atol=1e-12)
            steps = mref.step_shortfalls(G, bias, ids, rg, pg, lam, cosine)   # the reference's own sequence: margin 0 by construction
            assert all(abs(short) <= 1e-12 and e >= 0 for short, e in steps)


def test_lambda_one_is_the_prefix_and_lambda_zero_starts_at_position_zero():
    F = mref.exact_items(60, 9, 7)
    ids = _pool(60, 30, 5)
    r = np.sort(np.random.default_rng(5).integers(-9, 10, 30))[::-1].astype(np.float32)   # sorted, with ties: the pool of candidates()
    sims = mref.RowSims(F, 0, ids, False, "f32")
    picks, values = mref.mmr_greedy(r, sims.column, 1.0, 12)
    assert np.array_equal(picks, np.arange(12)) and np.array_equal(values, r[:12])
    picks, values = mref.mmr_greedy(r, sims.column, 0.0, 12)
    assert picks[0] == 0 and values[0] == 0                        # every v is 0 at step 0: the lowest position
    assert len(set(picks)) == 12


def test_duplicates_and_ties():
    F = mref.exact_items(20, 6, 3)
    F[4] = [1, 2, 0, -1, 3, 1]
    # all candidates identical: every sim is |x|^2, every v equal at every step -> position order
    ids = np.full(9, 4)
    sims = mref.RowSims(F, 0, ids, False, "f32")
    picks, values = mref.mmr_greedy(np.full(9, 2, dtype=np.float32), sims.column, 0.5, 9)
    assert np.array_equal(picks, np.arange(9))
    assert values[0] == 1.0 and (values[1:] == np.float32(1.0 - 0.5 * 16)).all()
    # all relevances equal, a duplicated id: the twin of the first pick is as similar as can be and goes last among equals
    ids = np.array([4, 7, 4, 9])
    picks, _ = mref.mmr_greedy(np.ones(4, dtype=np.float32), mref.RowSims(F, 0, ids, False, "f32").column, 0.25, 4)
    assert picks[0] == 0 and sorted(picks) == [0, 1, 2, 3]
    d = mref.RowSims(F, 0, ids, False, "int").column(0)
    assert d[2] == d[0] == 16 and np.argmax(picks == 2) >= np.argmax(picks == (1 if d[1] < 16 else 2))
    # -0.0 and +0.0 are one value: the lower position wins
    picks, _ = mref.mmr_greedy(np.array([-0.0, 0.0, -0.0], dtype=np.float32), mref.RowSims(F, 0, ids[:3], False, "f32").column, 1.0, 3)
    assert np.array_equal(picks, [0, 1, 2])


def test_intra_list_similarity_reference():
    F = mref.pow4_items(30, 17, 1, 11)
    ids = np.array([3, 15, 3, 8, 29, 0])                            # 15 = n // 2: the zero-norm row
    for cosine in (False, True):
        sims = mref.RowSims(F, 1, ids, cosine, "f32")
        M = sims.matrix().astype(np.float64)
        lower = np.tril_indices(len(ids), -1)
        mean, top = mref.ils_ref(sims, len(ids))
        assert mean == np.float32(M[lower].mean()) and top == np.float32(M[lower].max())
        m64, bm, t64, bt = mref.ils_bounds(F, 1, ids, cosine)
        assert abs(float(mean) - m64) <= bm and abs(float(top) - t64) <= bt
    assert mref.ils_ref(sims, 1) == (0, -np.inf) and mref.ils_ref(sims, 0) == (0, -np.inf)


# ----------------------------------------------------------------------------------------- the Python surface, before any GPU use
def _model(bias=False, users=True):
    from recmodel_amd import WMF
    m = WMF(num_items=30, num_users=20, dim=4, gamma=0.1, weighted=True, bias=bias)
    if users:
        m.users = np.random.default_rng(0).random((20, m.items.shape[1])).astype(np.float32)
    return m


def _no_gpu(monkeypatch):
    from recmodel_amd import _lib

    def touched():
        raise AssertionError("the GPU was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "require_gpu", touched)


GPU_TOUCHED = pytest.raises(AssertionError, match="GPU was touched")


@pytest.mark.parametrize("bias", (False, True))
def test_recommend_diverse_checks_come_before_the_gpu(monkeypatch, bias):
    from recmodel_amd import wmf_model
    _no_gpu(monkeypatch)
    m = _model(bias)
    hist = sp.random(3, 30, density=0.2, format="csr", random_state=1)
    for call, rows in ((m.recommend_diverse, [0, 1]), (m.recommend_diverse_for, hist)):
        with pytest.raises(ValueError, match="metric"):
            call(rows, metric="euclid")
        for bad in (0, -1, wmf_model.RECOMMEND_MAX_TOPN + 1):
            with pytest.raises(ValueError, match="topn"):
                call(rows, topn=bad)
        for bad in (0, wmf_model.MMR_MAX_POOL + 1):
            with pytest.raises(ValueError, match="pool"):
                call(rows, topn=1, pool=bad)
        with pytest.raises(ValueError, match="at least topn"):
            call(rows, topn=10, pool=9)
        for bad in (-0.01, 1.01, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="lam"):
                call(rows, lam=bad)
        with pytest.raises(ValueError, match="allow"):
            call(rows, allow=np.ones(29, dtype=bool))
        with GPU_TOUCHED:                                           # good arguments do reach the device
            call(rows, topn=wmf_model.RECOMMEND_MAX_TOPN, pool=wmf_model.MMR_MAX_POOL, lam=0.0, metric="dot")
        with GPU_TOUCHED:
            call(rows, topn=3, lam=1.0)
    with pytest.raises(IndexError):
        m.recommend_diverse([20])
    with pytest.raises(ValueError, match="exclude"):
        m.recommend_diverse([0], exclude=sp.csr_matrix((3, 30)))
    with pytest.raises(ValueError, match="count_rows"):
        m.recommend_diverse_for(sp.csr_matrix((3, 29)))
    assert wmf_model.WMF._mmr_arguments(10, None, 0.7, "cosine") == (10, 100, 0.7, True)
    assert wmf_model.WMF._mmr_arguments(128, None, 1, "dot") == (128, 1280, 1.0, False)
    assert wmf_model.MMR_MAX_POOL == wmf_model.CANDIDATES_MAX == 4096


def test_rerank_mmr_checks_come_before_the_gpu(monkeypatch):
    from recmodel_amd import wmf_model
    _no_gpu(monkeypatch)
    m = _model()
    ids, sc = np.arange(12).reshape(2, 6), np.ones((2, 6), dtype=np.float32)
    with pytest.raises(ValueError, match="metric"):
        m.rerank_mmr(ids, sc, metric="l2")
    with pytest.raises(ValueError, match="topn"):
        m.rerank_mmr(ids, sc, topn=129)
    with pytest.raises(ValueError, match="lam"):
        m.rerank_mmr(ids, sc, lam=2)
    with pytest.raises(ValueError, match="one shape"):
        m.rerank_mmr(ids, sc[:, :5])
    with pytest.raises(ValueError, match="one shape"):
        m.rerank_mmr(ids.reshape(2, 3, 2), sc.reshape(2, 3, 2))
    with pytest.raises(ValueError, match="integer"):
        m.rerank_mmr(sc, sc)
    with pytest.raises(ValueError, match="between 1 and"):
        m.rerank_mmr(np.zeros((1, 4097), dtype=np.int64), np.zeros((1, 4097), dtype=np.float32))
    with pytest.raises(ValueError, match="between 1 and"):
        m.rerank_mmr(np.zeros((2, 0), dtype=np.int64), np.zeros((2, 0), dtype=np.float32))
    for bad in (30, -2):
        with pytest.raises(IndexError):
            m.rerank_mmr(np.where(ids == 3, bad, ids), sc)
    with pytest.raises(ValueError, match="NaN"):
        m.rerank_mmr(ids, np.where(ids == 3, np.nan, sc))
    with pytest.raises(ValueError, match="pool_count"):
        m.rerank_mmr(ids, sc, pool_count=np.array([1, 2, 3]))
    with pytest.raises(ValueError, match="pool_count"):
        m.rerank_mmr(ids, sc, pool_count=np.array([1, 7]))
    with pytest.raises(ValueError, match="pool_count"):
        m.rerank_mmr(ids, sc, pool_count=np.array([-1, 2]))
    with pytest.raises(ValueError, match="pool_count"):
        m.rerank_mmr(ids, sc, pool_count=np.array([1.0, 2.0]))
    with GPU_TOUCHED:
        m.rerank_mmr(ids, sc, topn=128, lam=0, metric="dot", pool_count=np.array([0, 6]))
    with GPU_TOUCHED:
        m.rerank_mmr(np.array([3, 4, -1]), np.array([1.0, 0.5, -np.inf], dtype=np.float32))
    with pytest.raises(AttributeError, match="user factors"):
        _model(users=False).rerank_mmr(ids, sc)


def test_intra_list_similarity_checks_come_before_the_gpu(monkeypatch):
    from recmodel_amd import wmf_model
    _no_gpu(monkeypatch)
    m = _model(True)
    lists = np.array([[1, 2, 3], [4, -1, -1]])
    with pytest.raises(ValueError, match="metric"):
        m.intra_list_similarity(lists, metric="jaccard")
    with pytest.raises(ValueError, match="integer"):
        m.intra_list_similarity(lists.astype(np.float32))
    with pytest.raises(ValueError, match="width"):
        m.intra_list_similarity(np.zeros((2, wmf_model.ILS_MAX_WIDTH + 1), dtype=np.int64))
    with pytest.raises(ValueError, match="width"):
        m.intra_list_similarity(np.zeros((2, 0), dtype=np.int64))
    with pytest.raises(ValueError, match="width"):
        m.intra_list_similarity(np.zeros((2, 2, 2), dtype=np.int64))
    for bad in (30, -2):
        with pytest.raises(IndexError):
            m.intra_list_similarity(np.where(lists == 2, bad, lists))
    with GPU_TOUCHED:
        m.intra_list_similarity(lists)
    with GPU_TOUCHED:
        m.intra_list_similarity(np.zeros(wmf_model.ILS_MAX_WIDTH, dtype=np.int64), metric="dot")
    with pytest.raises(AttributeError, match="user factors"):
        _model(users=False).intra_list_similarity(lists)


# ------------------------------------------------------------------------------------------------------------ the C ABI
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build()
    from recmodel_amd import _lib
    return _lib.load()


P = ctypes.c_void_p(16)                                             # a non-null pointer that is never followed: every call is refused


def _mmr(lib, items=P, n_items=100, f=16, ld=16, bias=0, inv=None, pool_items=P, pool_scores=P, pool_count=None, n_rows=4, pool=32,
         lam=0.5, topn=10, out_items=P, out_scores=None, out_marginal=None, out_count=None):
    return lib.wmf_rerank_mmr(items, n_items, f, ld, bias, inv, pool_items, pool_scores, pool_count, n_rows, pool, lam, topn, out_items,
                              out_scores, out_marginal, out_count, None)


def _ils(lib, items=P, n_items=100, f=16, ld=16, bias=0, inv=None, lists=P, count=None, n_rows=4, width=10, out_mean=P, out_max=P):
    return lib.wmf_intra_list_similarity(items, n_items, f, ld, bias, inv, lists, count, n_rows, width, out_mean, out_max, None)


def test_every_refusal_of_the_c_entries(lib):
    from recmodel_amd import _lib
    bad_mmr = [dict(f=0), dict(f=261, ld=264), dict(ld=15), dict(ld=12), dict(f=16, ld=276), dict(items=None), dict(pool_items=None),
               dict(pool_scores=None), dict(out_items=None), dict(n_rows=0), dict(n_rows=-1), dict(n_items=0), dict(n_items=1 << 31),
               dict(pool=0), dict(pool=4097), dict(topn=0), dict(topn=129), dict(lam=-0.001), dict(lam=1.001), dict(lam=float("nan")),
               dict(lam=float("inf")), dict(lam=-float("inf"))]
    for kw in bad_mmr:
        assert _mmr(lib, **kw) == _lib.WMF_EINVAL, kw
        assert lib.wmf_last_error()
        with pytest.raises(ValueError):
            _lib.check(_mmr(lib, **kw))
    bad_ils = [dict(f=0), dict(ld=15), dict(f=16, ld=276), dict(items=None), dict(lists=None), dict(out_mean=None), dict(out_max=None),
               dict(n_rows=0), dict(n_items=0), dict(n_items=1 << 31), dict(width=0), dict(width=129)]
    for kw in bad_ils:
        assert _ils(lib, **kw) == _lib.WMF_EINVAL, kw


def test_resident_pool_formula(lib):
    """Pure host arithmetic: positive at every width, never growing with the leading dimension, 0 for a shape no kernel takes, and
    what DESIGN.md says about k = 128 + bias and k = 64."""
    for f in range(1, 261):
        base = lib.wmf_ld_for(f)
        got = [lib.wmf_rerank_mmr_resident_pool(f, ld) for ld in range(base, 273, 4)]
        assert all(1 <= g <= 4096 for g in got), f
        assert all(a >= b for a, b in zip(got, got[1:])), f
        # the rows and 16 bytes of state a candidate fit 160 KB; one more row would come within 4 KB of it (or the pool limit is reached)
        for ld, g in zip(range(base, 273, 4), got):
            assert g * (4 * ld + 16) <= 160 * 1024 and (g == 4096 or (g + 1) * (4 * ld + 16) > 156 * 1024), (f, ld, g)
    assert lib.wmf_rerank_mmr_resident_pool(129, 132) > 200 and lib.wmf_rerank_mmr_resident_pool(129, 132) < 1000
    assert lib.wmf_rerank_mmr_resident_pool(64, 64) >= 500
    assert lib.wmf_rerank_mmr_resident_pool(1, 4) == 4096
    for f, ld in ((0, 4), (5, 4), (16, 18), (261, 264), (16, 276)):
        assert lib.wmf_rerank_mmr_resident_pool(f, ld) == 0


def test_abi_table_has_the_new_symbols(lib):
    from recmodel_amd import _lib
    from recmodel_amd.engine import HipKernels
    for name in ("wmf_rerank_mmr", "wmf_rerank_mmr_resident_pool", "wmf_intra_list_similarity"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.SIGNATURES["wmf_rerank_mmr"][1][11] is ctypes.c_float      # lambda travels as a float32
    assert lib.wmf_rerank_mmr_resident_pool.restype is ctypes.c_int64
    for method in ("rerank_mmr", "rerank_mmr_resident_pool", "intra_list_similarity"):
        assert callable(getattr(HipKernels, method))
