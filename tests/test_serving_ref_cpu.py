"""The host references of tests/serving_ref.py against the oracle, on tie-free inputs, so that the GPU tests of
tests/test_gpu_serving.py compare the kernels with something that was itself checked (no GPU needed here)."""
import numpy as np
import scipy.sparse as sp

import serving_ref as ref
from oracle import wmf_oracle as orc


def _factors(n_users, n_items, f, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n_users, f)).astype(np.float32), rng.standard_normal((n_items, f)).astype(np.float32)


def test_scores_match_oracle_predict():
    Uf, If = _factors(20, 90, 13, 1)
    rng = np.random.default_rng(2)
    users, items = rng.integers(0, 20, 200), rng.integers(0, 90, 200)
    for bias in (False, True):
        want = orc.predict(Uf.astype(np.float64), If.astype(np.float64), users, items, bias)
        np.testing.assert_allclose(ref.scores_f64(Uf, If, users, items, bias), want, rtol=1e-14, atol=1e-14)
        np.testing.assert_allclose(ref.scores_f64(Uf, If, [4], items, bias),
                                   orc.predict(Uf.astype(np.float64), If.astype(np.float64), [4], items, bias), rtol=1e-14, atol=1e-14)
        Ue, Ie = ref.exact_factors(20, 13, 3), ref.exact_factors(90, 13, 4)
        want = orc.predict(Ue.astype(np.float64), Ie.astype(np.float64), users, items, bias)
        assert np.array_equal(ref.scores_int(Ue, Ie, users, items, bias), want.astype(np.int64)) and np.array_equal(want, np.rint(want))
        S = ref.score_matrix_int(Ue, Ie, users[:7], items[:30], bias)
        for r in range(7):
            assert np.array_equal(S[r], ref.scores_int(Ue, Ie, users[r:r + 1], items[:30], bias))
        # the bound is positive and far above the float64 reference's own rounding
        assert (ref.score_bound(Uf, If, users, items, bias) > 0).all()


def test_stable_topn_matches_oracle_rank_without_ties():
    Uf, If = _factors(5, 400, 9, 5)
    Ud, Id = Uf.astype(np.float64), If.astype(np.float64)
    cand = np.random.default_rng(6).permutation(400)[:333]
    for bias in (False, True):
        s = ref.scores_f64(Uf, If, [2], cand, bias)
        assert len(np.unique(s)) == len(s)                           # tie-free: the oracle's order is then determined
        for topn in (1, 7, 166, 167, 332, 333):                      # both of the oracle's branches, both of stable_topn's
            want = orc.rank(Ud, Id, cand, [2], topn=topn, bias=bias)
            assert np.array_equal(cand[ref.stable_topn(s, topn)], want), (bias, topn)


def test_stable_topn_keeps_candidate_order_among_ties():
    s = np.array([1, 3, 3, -2, 3, 1, 0, 1], dtype=np.int64)
    assert ref.stable_topn(s, 8).tolist() == [1, 2, 4, 0, 5, 7, 6, 3]
    assert ref.stable_topn(s, 1).tolist() == [1]                    # the partition shortcut
    assert ref.stable_topn(s.astype(np.float32), 4).tolist() == [1, 2, 4, 0]
    big = np.tile(s, 50)
    for topn in (1, 2, 60, 99, 100, 400):
        assert np.array_equal(ref.stable_topn(big, topn), np.argsort(-big, kind="stable")[:topn])
    v = np.array([0.0, -np.inf, np.inf, -0.0, 3e38, np.inf], dtype=np.float32)
    assert ref.stable_topn(v, 6).tolist() == [2, 5, 4, 0, 3, 1]


def test_hit_counts_match_oracle_eval_topn():
    n_users, n_items, f, rand_sampled = 30, 500, 7, 50
    Uf, If = _factors(n_users, n_items, f, 7)
    rng = np.random.default_rng(8)
    rows = np.repeat(np.arange(n_users), rng.integers(0, 4, n_users))
    cols = np.concatenate([rng.choice(n_items, c, replace=False) for c in np.bincount(rows, minlength=n_users)]).astype(np.int64)
    test_mat = sp.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(n_users, n_items))
    topn = np.array([1, 5, 10])
    for bias in (False, True):
        _, want = orc.eval_topn(Uf.astype(np.float64), If.astype(np.float64), test_mat, topn, rand_sampled=rand_sampled,
                                random_state=11, bias=bias, return_hits=True)
        # the oracle's draws, in its order (oracle/wmf_oracle.py, eval_topn): one candidate row and one slot per user with entries
        np.random.seed(11)
        s_true, s_cand, slot = [], [], []
        for user in range(n_users):
            test_idx = test_mat.indices[test_mat.indptr[user]:test_mat.indptr[user + 1]]
            if len(test_idx) == 0:
                continue
            cand = np.random.randint(0, n_items, size=rand_sampled + 1)
            sl = np.random.randint(0, rand_sampled - 2 * topn.max())
            for item in test_idx:
                s_true.append(ref.scores_f64(Uf, If, [user], [item], bias)[0])
                s_cand.append(ref.scores_f64(Uf, If, [user], cand, bias))
                slot.append(sl)
        got = ref.hit_counts(np.array(s_true), np.array(s_cand), np.array(slot), topn)
        assert np.array_equal(got, want.astype(np.int64)), (bias, got, want)
        assert got[0] <= got[1] <= got[2] and 0 < got[2] < len(s_true)   # the comparison is not vacuous
    assert ref.hit_counts(np.zeros(0), np.zeros((0, 5)), np.zeros(0, dtype=np.int64), [0, 3]).tolist() == [0, 0]
    # strictly higher: a tie does not count, topn = 0 never hits
    assert ref.hit_counts(np.array([2]), np.array([[2, 9, 2, 1]]), np.array([1]), [0, 1, 2]).tolist() == [0, 1, 1]
    assert ref.hit_counts(np.array([2]), np.array([[3, 9, 2, 1]]), np.array([1]), [0, 1, 2]).tolist() == [0, 0, 1]


def test_eval_sums_match_oracle_eval_prec():
    n_users, n_items, f = 25, 60, 11
    Uf, If = _factors(n_users, n_items, f, 9)
    rng = np.random.default_rng(10)
    M = sp.random(n_users, n_items, density=0.2, random_state=3, format="csr", dtype=np.float64)
    M.data = rng.standard_normal(M.nnz).astype(np.float32).astype(np.float64)
    M.data[::7] = 0.0                                                # stored zeros: skipped by both
    M.data[3::7] = -0.0
    rows = ref.csr_rows(M.indptr)
    for bias in (False, True):
        sq, ab, cnt = ref.eval_sums(ref.scores_f64(Uf, If, rows, M.indices, bias), M.data)
        assert cnt == int((M.data != 0).sum()) < M.nnz
        Ud, Id = Uf.astype(np.float64), If.astype(np.float64)
        np.testing.assert_allclose(sq / cnt, orc.eval_prec(Ud, Id, M, bias, "mse"), rtol=1e-12)
        np.testing.assert_allclose(ab / cnt, orc.eval_prec(Ud, Id, M, bias, "mae"), rtol=1e-12)
    Ue, Ie = ref.exact_factors(n_users, f, 1), ref.exact_factors(n_items, f, 2)
    vals = rng.integers(-5, 6, M.nnz).astype(np.float32)
    si = ref.scores_int(Ue, Ie, rows, M.indices, True)
    sq, ab, cnt = ref.eval_sums(si, vals)
    fsq, fab, fcnt = ref.eval_sums(si.astype(np.float64), vals)
    assert isinstance(sq, int) and (sq, ab, cnt) == (fsq, fab, fcnt)
    assert ref.eval_sums(si, np.zeros(M.nnz, dtype=np.float32)) == (0, 0, 0)


def test_exact_class_stays_below_2_24_at_the_widest_factors():
    f = ref.WMF_MAX_F
    Ue, Ie = ref.exact_factors(64, f, 1), ref.exact_factors(300, f, 2)
    assert Ue.dtype == np.float32 and np.abs(Ue).max() == 3 and np.abs(Ie).max() == 3 and np.array_equal(Ue, np.rint(Ue))
    for bias in (False, True):
        S = ref.score_matrix_int(Ue, Ie, np.arange(64), np.arange(300), bias)
        assert np.abs(S).max() < 2 ** 24
    # the worst the class allows: every entry +-3, so every partial sum of |products| and biases is below 2^24 as well
    assert 9 * f < 2 ** 24 and 9 * (f - 1) + 6 < 2 ** 24


def test_histogram_boundary_levels_have_the_bin_properties():
    values, levels, counts = ref.hist_case(0)
    assert len(values) == counts.sum() and counts.min() >= 1 and counts.max() <= 40
    assert np.array_equal(np.unique(values), np.unique(levels)) and (np.diff(levels) > 0).all()
    assert all(ref.hist_bin_properties(levels).values()), ref.hist_bin_properties(levels)
    key = ref.rank_key(levels)
    assert (np.diff(key.astype(np.int64)) > 0).all()                # the key is order preserving
    bins = key >> 20
    assert bins[6] == bins[7]                                        # 1 and 1 + 2^-10: one bin
    assert bins[8] != bins[9] and bins[8] >> 4 == bins[9] >> 4       # 1.125 and 1.25: two bins of one group
    assert bins[0] >> 4 == 0 and bins[0] > 0                         # -inf: group 0, not its lowest bin
    assert not ref.hist_bin_properties([1.0, 2.0, 4.0])["bin_in_group_0"]
