"""The posterior of a folded-in row without a GPU: tests/posterior_ref.py against dense float64 algebra and the oracle-checked
fold-in, the hash and its variates, the statistic the GPU draws are held to on the reference's own draws, the float32
restatements, and the argument checks of the three entry points and the model calls."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import foldin_ref
import posterior_ref as ref
import sample_ref
from conftest import ROOT


def _small_case(bias, seed):
    """tests/test_foldin_cpu.py's: f = 6 (+ bias column), 25 items, an empty row, a stored zero, a duplicate, a row longer than f."""
    rng = np.random.default_rng(seed)
    m, f = 25, 6 + bias
    Y = rng.random((m, f))
    degrees = [4, 0, 3, 15, 1, 2]
    indptr = np.concatenate([[0], np.cumsum(degrees)]).astype(np.int64)
    indices = np.concatenate([rng.choice(m, d, replace=False) for d in degrees]).astype(np.int32)
    values = 10 * np.log1p(rng.integers(1, 6, len(indices)).astype(np.float64))
    values[2] = 0.0
    indices[indptr[2] + 1] = indices[indptr[2]]
    return Y, indptr, indices, values


# ------------------------------------------------------------------------------------------------------- the definitions
@pytest.mark.parametrize("bias", [0, 1])
def test_a_draw_has_the_posterior_covariance_and_the_fold_in_as_its_mean(bias):
    """x~ = x_u + sigma M xi with M M^T = inv(A_u): read M off the reference by drawing with the unit vectors as xi."""
    Y, indptr, indices, values = _small_case(bias, 31 + bias)
    lam, sigma, f, n = 0.3, 0.7, Y.shape[1], len(indptr) - 1
    x = foldin_ref.ref64(Y, bias, lam, indptr, indices, values)
    xi = np.broadcast_to(np.vstack([np.zeros((1, f)), np.eye(f)]), (n, f + 1, f))
    d = ref.draws64(Y, bias, lam, indptr, indices, values, xi, sigma)
    Yt, _ = ref.tilde(Y, bias)
    for u in range(n):
        lo, hi = indptr[u], indptr[u + 1]
        A, _ = ref.row_system(Y, bias, lam, indices[lo:hi], values[lo:hi])          # an empty row: the prior's G~ + lambda I
        assert np.abs(d[u, 0] - x[u]).max() <= 1e-11 * max(1.0, np.abs(x[u]).max())
        M = (d[u, 1:] - d[u, 0]).T / sigma                                           # column k: the image of unit vector k
        assert np.abs(sigma ** 2 * M @ M.T - sigma ** 2 * np.linalg.inv(A)).max() <= 1e-10 * np.abs(np.linalg.inv(A)).max()
    assert (d[1, 0] == 0).all()


@pytest.mark.parametrize("bias", [0, 1])
def test_mean_is_the_score_of_the_fold_in_and_var_a_dense_solve(bias):
    Y, indptr, indices, values = _small_case(bias, 41 + bias)
    lam, n, m = 0.3, len(indptr) - 1, len(Y)
    targets = np.tile(np.arange(m, dtype=np.int32), (n, 1))
    targets[:, 5] = -1
    mean, var, M = ref.scores64(Y, bias, lam, indptr, indices, values, targets)
    x = foldin_ref.ref64(Y, bias, lam, indptr, indices, values)                      # (the oracle's half step: test_foldin_cpu.py)
    Yt, beta = ref.tilde(Y, bias)
    want = Yt @ x.T + beta[:, None]
    ok = targets[0] >= 0
    assert np.abs(mean[:, ok] - want.T[:, ok]).max() <= 1e-10 and (mean[:, 5] == 0).all() and (var[:, 5] == 0).all()
    W = ref.whitening(Y, bias, lam)
    for u in range(n):
        lo, hi = indptr[u], indptr[u + 1]
        A, _ = ref.row_system(Y, bias, lam, indices[lo:hi], values[lo:hi])
        dense = np.diag(Yt @ np.linalg.inv(A) @ Yt.T)
        assert np.abs(var[u, ok] - dense[ok]).max() <= 1e-10 * dense.max() and (var[u, ok] > 0).all()
        assert (np.abs(mean[u, ok] - beta[ok]) <= M[u, ok] * (1 + 1e-9)).all()       # |z . c| <= |z| |c|
    assert np.abs(var[1, ok] - ((Yt @ W) ** 2).sum(axis=1)[ok]).max() <= 1e-10       # an empty row: the prior variance |q_i|^2
    # in whitened coordinates, as the kernel computes them: z = L^-1 q, c = L^-1 b
    u = 3
    j = indices[indptr[u]:indptr[u + 1]]
    w = values[indptr[u]:indptr[u + 1]] - beta[j]
    Q = Yt[j] @ W
    L = np.linalg.cholesky(np.eye(Y.shape[1]) + Q.T @ (Q * w[:, None]))
    Z = np.linalg.solve(L, (Yt @ W).T).T
    c = np.linalg.solve(L, (w + 1) @ Q)
    assert np.abs((Z * Z).sum(axis=1)[ok] - var[u, ok]).max() <= 1e-10 and np.abs((Z @ c + beta)[ok] - mean[u, ok]).max() <= 1e-10


# ------------------------------------------------------------------------------------------------------- the noise
def test_hash_in_python_integers_and_in_numpy_agree():
    rng = np.random.default_rng(5)
    seeds = [0, 1, 2 ** 64 - 1, 123456789]
    for seed in seeds:
        streams = np.array([0, 1, 2 ** 64 - 1, 2 ** 63] + [int(v) for v in rng.integers(0, 2 ** 62, 20)], dtype=np.uint64)
        draws = np.array([0, ref.MAX_DRAWS - 1, 2 ** 31 - 1, 7] + [int(v) for v in rng.integers(0, ref.MAX_DRAWS, 20)])
        comps = np.array([0, ref.MAX_F - 1, 2 ** 31 - 1, 3] + [int(v) for v in rng.integers(0, ref.MAX_F, 20)])
        k1, k2 = ref.normal_k(seed, streams, draws, comps)
        for i in range(len(streams)):
            assert (int(k1[i]), int(k2[i])) == ref.normal_k_int(seed, int(streams[i]), int(draws[i]), int(comps[i]))
        assert k1.max() < 2 ** 23 and k2.max() < 2 ** 23
    # the row prefix is the Gumbel noise's: the same (seed, stream) gives the same a
    with np.errstate(over="ignore"):
        a = sample_ref.mix(np.uint64(7) + sample_ref.GOLDEN * np.uint64(4))
    assert int(a) == ref.mix_int(7 + ref.GOLDEN_INT * 4)


def test_key_ranges_are_disjoint_from_the_gumbel_noise():
    """The Gumbel noise hashes item + 1 for a 32-bit id: at most 2^32.  A normal variate hashes 2^32 (draw + 1) + component + 1 >=
    2^32 + 1, below 2^64 for draw < 2^31 (no wrap), and distinct (draw, component) pairs give distinct keys."""
    gumbel_max = (2 ** 32 - 1) + 1
    assert ref.normal_key_int(0, 0) == 2 ** 32 + 1 > gumbel_max
    assert ref.normal_key_int(2 ** 31 - 1, 2 ** 31 - 1) < 2 ** 64
    assert ref.normal_key_int(ref.MAX_DRAWS - 1, ref.MAX_F - 1) < 2 ** 45
    assert ref.normal_key_int(3, 2 ** 31 - 1) < ref.normal_key_int(4, 0)            # a component never reaches the next draw's keys
    keys = {ref.normal_key_int(d, c) for d in range(64) for c in range(ref.MAX_F)}
    assert len(keys) == 64 * ref.MAX_F


def test_variates_stay_inside_the_documented_bound_and_have_normal_moments():
    assert abs(ref.XI_BOUND - 5.768) < 1e-3
    corners = ref.xi64(np.array([0, 0, 2 ** 23 - 1]), np.array([0, 2 ** 22, 0]))
    assert np.abs(corners).max() <= ref.XI_BOUND and abs(corners[0]) > 5.76 and corners[1] < -5.76
    k2 = np.arange(2 ** 23)
    assert (np.cos(np.pi * (2.0 * k2[::4097] + 1.0) * 2.0 ** -23) != 0).all()
    N = 2 ** 20
    xi = ref.xi_block(3, 17, N // 256, 256).ravel()
    assert np.abs(xi).max() <= ref.XI_BOUND
    # moments of N independent standard normals: the mean has sd 1 / sqrt(N), the second moment sqrt(2 / N), the fourth sqrt(96 / N);
    # 4.5 standard deviations each
    m1, m2, m4 = xi.mean(), (xi ** 2).mean(), (xi ** 4).mean()
    print(f"xi over 2^20 keys: mean {m1:.2e}, variance {m2:.5f}, fourth moment {m4:.4f}")
    assert abs(m1) <= 4.5 / np.sqrt(N) and abs(m2 - 1) <= 4.5 * np.sqrt(2 / N) and abs(m4 - 3) <= 4.5 * np.sqrt(96 / N)
    # components of one draw, and draws of one component, are uncorrelated
    blk = ref.xi_block(9, 2, 4096, 8)
    corr = np.corrcoef(blk.T)
    assert np.abs(corr - np.eye(8)).max() <= 4.5 / np.sqrt(4096)


@pytest.mark.parametrize("bias", [0, 1])
def test_the_references_own_draws_pass_the_covariance_gate(bias):
    """The seeds of the GPU test: the float64 draws under the float64 variates of the hash lie under the gate the device's are
    held to, and a wrong covariance does not."""
    c = ref.stat_case(bias)
    assert c["f"] == 5 and np.diff(c["indptr"]).tolist() == [7]
    for seed in ref.STAT_SEEDS:
        stat = ref.reference_statistic(c, seed)
        print(f"bias {bias} seed {seed}: statistic {stat:.2f} (gate {ref.CHI2_15_999})")
        assert 0 < stat < ref.CHI2_15_999
    Yf = c["Y"][:, :5]
    X = ref.draws64(Yf, bias, c["lam"], c["indptr"], c["indices"], c["values"], ref.xi_block(ref.STAT_SEEDS[0], 0, 4096, 5)[None],
                    ref.STAT_SIGMA)[0]
    assert ref.covariance_statistic(X, c["x"], 1.1 * c["cov"]) > ref.CHI2_15_999    # sigma off by 5 %: caught
    assert ref.covariance_statistic(X, c["x"], np.diag(np.diag(c["cov"]))) > ref.CHI2_15_999


# ------------------------------------------------------------------------------------------------------- the restatements
def test_restated_draws_at_sigma_zero_are_the_restated_fold_in():
    for name in ("width_f5_b0_x4", "gauss_f16_b0", "width_f31_b1_x0"):
        c = foldin_ref.case(name)
        Yf, n, f = c["Y"][:, :c["f"]], len(c["indptr"]) - 1, c["f"]
        want = foldin_ref.restated32(Yf, c["bias"], c["W32"], c["indptr"], c["indices"], c["values"])
        got = ref.restated_draws32(Yf, c["bias"], c["W32"], c["indptr"], c["indices"], c["values"], np.ones((n, 2, f), dtype=np.float32), 0.0)
        assert np.array_equal(got[:, 0].view(np.uint32), want.view(np.uint32)) and np.array_equal(got[:, 1].view(np.uint32), want.view(np.uint32))


def test_restatements_match_the_definitions():
    c = foldin_ref.case("gauss_f16_b0")
    Yf, n, f = c["Y"][:, :c["f"]], len(c["indptr"]) - 1, c["f"]
    xi = np.stack([ref.xi_block(4, u, 3, f) for u in range(n)]).astype(np.float32)
    d64 = ref.draws64(Yf, c["bias"], c["lam"], c["indptr"], c["indices"], c["values"], xi.astype(np.float64), 0.5)
    d32 = ref.restated_draws32(Yf, c["bias"], c["W32"], c["indptr"], c["indices"], c["values"], xi, 0.5)
    err = ref.draw_errors(d32, d64)
    assert err.max() <= 1e-5, err.max()
    tg = ref.targets_for(c, 17)
    mean, var, M = ref.scores64(Yf, c["bias"], c["lam"], c["indptr"], c["indices"], c["values"], tg)
    m32, v32 = ref.restated_scores32(Yf, c["bias"], c["W32"], c["indptr"], c["indices"], c["values"], tg)
    assert ref.score_errors(v32, var, var).max() <= 1e-5 and ref.score_errors(m32, mean, M).max() <= 1e-5
    assert (v32[tg < 0] == 0).all() and (m32[tg < 0] == 0).all() and (v32[tg >= 0] > 0).all()
    assert np.array_equal(v32[:, 0], v32[:, -1]) and np.array_equal(m32[:, 0], m32[:, -1])      # the same item twice
    # a failed row: NaN in its non-empty slots
    Y = np.eye(6, 4, dtype=np.float32)
    indptr, indices = np.array([0, 2, 2, 3]), np.array([0, 1, 2], dtype=np.int32)
    values = np.array([3.0, -2.0, 3.0], dtype=np.float32)
    tg = np.array([[0, -1], [2, 3], [2, 0]], dtype=np.int32)
    m32, v32 = ref.restated_scores32(Y, 0, np.eye(4, dtype=np.float32), indptr, indices, values, tg)
    assert np.isnan(m32[0, 0]) and np.isnan(v32[0, 0]) and m32[0, 1] == 0 and v32[0, 1] == 0
    assert v32[1].tolist() == [1.0, 1.0] and m32[1].tolist() == [0.0, 0.0]           # an empty row: the prior, |q|^2 = 1
    assert v32[2].tolist() == [0.25, 1.0] and m32[2].tolist() == [1.0, 0.0]          # 1 / (1 + 3), and (3 + 1) / (1 + 3)
    d32 = ref.restated_draws32(Y, 0, np.eye(4, dtype=np.float32), indptr, indices, values, np.ones((3, 1, 4), dtype=np.float32), 2.0)
    assert np.isnan(d32[0]).all() and d32[1, 0].tolist() == [2.0] * 4 and d32[2, 0].tolist() == [2.0, 2.0, 2.0, 2.0]


def test_orthogonal_closed_forms():
    c, parts = ref.orthogonal_parts()
    Yf = c["Y"][:, :c["f"]]
    n, f = len(c["indptr"]) - 1, c["f"]
    xi = np.stack([ref.xi_block(8, u, 2, f) for u in range(n)]).astype(np.float32)
    d64 = ref.draws64(Yf, 0, c["lam"], c["indptr"], c["indices"], c["values"], xi.astype(np.float64), 0.5)
    tg = np.tile(np.arange(c["m"], dtype=np.int32), (n, 1))
    mean, var, _ = ref.scores64(Yf, 0, c["lam"], c["indptr"], c["indices"], c["values"], tg)
    for u in range(n):
        for a in range(f):
            want = float(ref.orthogonal_exact_draw(parts, u, a, 0.5, xi[u, 1, a]))
            assert abs(d64[u, 1, a] - want) <= 1e-6 * max(abs(want), 1e-3)          # (W32 is W_white rounded to float32)
        for i in range(c["m"]):
            em, ev = ref.orthogonal_exact_score(c, parts, u, i)
            assert abs(var[u, i] - float(ev)) <= 1e-6 * float(ev) and abs(mean[u, i] - float(em)) <= 1e-6 * max(float(em), 1e-3)
            assert (em == 0) == (not parts[(u, int(c["axis"][i]))][3])
    assert abs(float(ref.sqrt_fraction(ref.Fraction(2))) - 2 ** 0.5) < 1e-15


# ------------------------------------------------------------------------------------------------------- argument checks
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build()
    from recmodel_amd import _lib
    return _lib.load()


def test_abi_table_and_workspace_formulas(lib):
    from recmodel_amd import _lib, wmf_model
    names = ("wmf_posterior_draw_workspace_bytes", "wmf_posterior_draw_rows", "wmf_posterior_score_workspace_bytes",
             "wmf_posterior_score_rows", "wmf_posterior_noise")
    header = open(os.path.join(ROOT, "include", "wmf_hip.h")).read()
    for name in names:
        assert name in _lib.SIGNATURES and hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, header)
    assert len(_lib.SIGNATURES["wmf_posterior_draw_rows"][1]) == 19 and len(_lib.SIGNATURES["wmf_posterior_score_rows"][1]) == 18
    for macro, value in (("WMF_POSTERIOR_MAX_DRAWS", wmf_model.POSTERIOR_MAX_DRAWS), ("WMF_POSTERIOR_MAX_TARGETS", wmf_model.POSTERIOR_MAX_TARGETS)):
        assert int(re.search(r"#define %s (\d+)" % macro, header).group(1)) == value == 4096
    assert ref.MAX_DRAWS == ref.MAX_TARGETS == 4096
    # a small constant (every width fits LDS), whatever the shape
    for n, f, k in ((0, 1, 1), (10, 16, 1), (1 << 20, 260, 4096)):
        assert lib.wmf_posterior_draw_workspace_bytes(n, f, k) == lib.wmf_posterior_score_workspace_bytes(n, f, k) == 256
    # the LDS budget of the header's widest model: the triangle of f + 1 rows, 16 slots, 8 staged rows and dinv, under 160 KB
    f = ref.MAX_F
    assert ((f + 1) * (f + 2) // 2 + 25 * f) * 4 + 160 <= 160 * 1024


def test_entry_points_check_their_arguments(lib):
    from recmodel_amd import _lib
    d = ctypes.c_void_p(16)
    draw_args = (("Y", d), ("m", 100), ("f", 16), ("ld", 16), ("bias", 0), ("W", d), ("indptr", d), ("indices", d), ("values", d), ("n", 10),
                 ("n_draws", 4), ("sigma", 1.0), ("seed", 5), ("row_stream", None), ("X", d), ("fail", d), ("ws", d), ("ws_bytes", 1 << 30),
                 ("stream", None))
    score_args = draw_args[:10] + (("targets", d), ("n_targets", 4), ("mean", d), ("var", d), ("fail", d), ("ws", d), ("ws_bytes", 1 << 30),
                                   ("stream", None))
    draw = lambda **kw: lib.wmf_posterior_draw_rows(*[kw.get(k, v) for k, v in draw_args])    # noqa: E731
    score = lambda **kw: lib.wmf_posterior_score_rows(*[kw.get(k, v) for k, v in score_args])  # noqa: E731
    shared = [dict(f=0), dict(f=261), dict(ld=15), dict(ld=12), dict(ld=276, f=260), dict(m=0), dict(m=1 << 31), dict(n=-1), dict(n=1 << 31),
              dict(ws_bytes=255), dict(Y=None), dict(W=None), dict(indptr=None), dict(indices=None), dict(values=None), dict(fail=None),
              dict(ws=None)]
    for bad in shared + [dict(n_draws=0), dict(n_draws=-1), dict(n_draws=4097), dict(n=1 << 19, n_draws=4096), dict(n=(1 << 31) - 1, n_draws=2),
                         dict(sigma=-1.0), dict(sigma=-1e-30), dict(sigma=float("inf")), dict(sigma=float("nan")), dict(X=None)]:
        assert draw(**bad) == _lib.WMF_EINVAL, bad
    for bad in shared + [dict(n_targets=0), dict(n_targets=-1), dict(n_targets=4097), dict(targets=None), dict(mean=None, var=None)]:
        assert score(**bad) == _lib.WMF_EINVAL, bad
    assert b"workspace" in (draw(ws_bytes=0), lib.wmf_last_error())[1] and b"sigma" in (draw(sigma=-2.0), lib.wmf_last_error())[1]
    assert b"2^31" in (draw(n=1 << 19, n_draws=4096), lib.wmf_last_error())[1]
    # no rows: nothing is launched, whatever is legal otherwise -- sigma 0, a stream array, one score output, the largest counts
    assert draw(n=0) == draw(n=0, sigma=0.0, row_stream=d, n_draws=4096) == _lib.WMF_OK
    assert score(n=0) == score(n=0, mean=None) == score(n=0, var=None, n_targets=4096) == _lib.WMF_OK
    noise = lambda **kw: lib.wmf_posterior_noise(*[kw.get(k, v) for k, v in (  # noqa: E731
        ("seed", 1), ("row_stream", None), ("draws", d), ("components", d), ("n", 5), ("xi", d), ("k", d), ("stream", None))])
    for bad in (dict(n=-1), dict(draws=None), dict(components=None), dict(xi=None, k=None)):
        assert noise(**bad) == _lib.WMF_EINVAL, bad
    assert noise(n=0) == noise(n=0, xi=None) == noise(n=0, k=None, row_stream=d) == _lib.WMF_OK


def test_model_methods_check_their_arguments_before_the_gpu(monkeypatch):
    from recmodel_amd import WMF, _lib, wmf_model

    def touched():
        raise AssertionError("the GPU was asked for before the arguments were checked")
    monkeypatch.setattr(_lib, "require_gpu", touched)
    C = sp.random(4, 5, density=0.5, format="csr", random_state=0)
    full = sp.random(6, 5, density=0.5, format="csr", random_state=1)
    tg = np.zeros((4, 3), dtype=np.int64)

    def calls(m):
        return ((m.posterior_draws, (C,)), (m.recommend_thompson_for, (C,)), (m.recommend_thompson, ([0, 1], full)),
                (m.score_posterior, (C, tg)), (m.recommend_ucb_for, (C,)))
    m = WMF(num_items=5, num_users=6, dim=2, gamma=0.1, weighted=False)
    m.users = np.zeros((6, 2), dtype=np.float32)
    for method, args in calls(m):
        with pytest.raises(ValueError):
            method(*args)                                          # not the weighted branch
    m = WMF(num_items=5, num_users=6, dim=2, gamma=0.1, weighted=True)
    m.users = np.zeros((6, 2), dtype=np.float32)
    for method, args in calls(m):
        with pytest.raises(AssertionError):
            method(*args)                                          # well-formed: the next thing it does is ask for the GPU
        with pytest.raises(ValueError):
            method(*args, pre_process_count="sqrt")
    wrong = sp.random(4, 6, density=0.5, format="csr", random_state=0)
    for method in (m.posterior_draws, m.recommend_thompson_for, m.recommend_ucb_for):
        for bad in (wrong, C.toarray()):
            with pytest.raises(ValueError):
                method(bad)
    for kw in (dict(draws=0), dict(draws=wmf_model.POSTERIOR_MAX_DRAWS + 1), dict(sigma=-1), dict(sigma=float("nan")), dict(sigma=float("inf")),
               dict(seed=-1), dict(seed=2 ** 64), dict(seed=1.5), dict(streams=[1, 2, 3]), dict(streams=[0, 1, 2, -1]),
               dict(streams=[0.5, 1, 2, 3]), dict(streams=np.zeros((4, 1), dtype=np.int64))):
        with pytest.raises(ValueError):
            m.posterior_draws(C, **kw)
    with pytest.raises(AssertionError):
        m.posterior_draws(C, draws=wmf_model.POSTERIOR_MAX_DRAWS, sigma=0, seed=2 ** 64 - 1, streams=[0, 2 ** 64 - 1, 5, 5])
    for kw in (dict(topn=0), dict(topn=wmf_model.CANDIDATES_MAX + 1), dict(sigma=-0.5), dict(seed=True), dict(streams=[1]),
               dict(allow=np.ones(4, dtype=bool)), dict(allow=np.ones((2, 5), dtype=bool))):
        with pytest.raises(ValueError):
            m.recommend_thompson_for(C, **kw)
    with pytest.raises(AssertionError):
        m.recommend_thompson_for(C, topn=wmf_model.CANDIDATES_MAX)
    with pytest.raises(IndexError):
        m.recommend_thompson([6], full)
    for bad in (C, full.toarray(), None):
        with pytest.raises(ValueError):
            m.recommend_thompson([0], bad)
    with pytest.raises(ValueError):
        m.recommend_thompson([0, 1], full, streams=[1, 2, 3])
    for bad in (np.zeros((3, 3), dtype=np.int64), np.zeros(4, dtype=np.int64), np.zeros((4, 3)), np.full((4, 3), 5), np.full((4, 3), -2)):
        with pytest.raises(ValueError):
            m.score_posterior(C, bad)
    with pytest.raises(AssertionError):
        m.score_posterior(C, np.array([[0, 4, -1]] * 4))
    for kw in (dict(topn=0), dict(topn=5, pool=4), dict(pool=0), dict(pool=wmf_model.CANDIDATES_MAX + 1), dict(topn=wmf_model.CANDIDATES_MAX + 1),
               dict(c=-1), dict(c=float("nan")), dict(c=float("inf")), dict(allow=np.ones(4, dtype=bool))):
        with pytest.raises(ValueError):
            m.recommend_ucb_for(C, **kw)
    with pytest.raises(AssertionError):
        m.recommend_ucb_for(C, topn=3, pool=wmf_model.CANDIDATES_MAX, c=0)


def test_no_product_file_names_the_test_infrastructure():
    for path in ("recmodel_amd/csrc/wmf_posterior.hip", "recmodel_amd/csrc/wmf_noise.h", "recmodel_amd/wmf_model.py", "include/wmf_hip.h",
                 "tools/posterior_lab.py"):
        assert "oracle" not in open(os.path.join(ROOT, path)).read().replace("test infrastructure", ""), path
