"""The contributions of a user's history without a GPU: tests/explain_ref.py against the oracle's fold-in (total = predict on
recompute_factors[_bias]) and the reference's own goldens, the caps that keep every GPU gate meaningful, and the argument
checks of wmf_explain_rows and WMF.explain."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import explain_ref as ref
from conftest import csr_from, load_golden
from oracle import wmf_oracle as orc

# The largest pair error the float32 restatement may have against float64 on the inputs of a family: 1.5 x the largest figure
# measured on the CPU for the committed cases (width 1.15e-4, gauss 8.6e-6, w1e3 5.1e-4, zeros 8.8e-6, dup 1.5e-5, eqbias 5.8e-6,
# neg 3.0e-6, targets 9.5e-6, long 1.5e-6, grid 5.0e-5).  A gate is 4 x the pair's figure + 8 ulps, so no gate exceeds
# 4 x cap + 8 ulps: none is vacuous.
RESTATED_CAP = {"width": 1.8e-4, "gauss": 1.3e-5, "w1e3": 7.7e-4, "zeros": 1.4e-5, "dup": 2.3e-5, "eqbias": 8.7e-6, "neg": 4.5e-6,
                "targets": 1.5e-5, "long": 2.3e-6, "grid": 7.5e-5}


def _small_case(bias, seed):
    """f = 6 (+ bias column), 25 items: an empty row, a stored zero, a duplicate entry, a row longer than f."""
    rng = np.random.default_rng(seed)
    m, f = 25, 6 + bias
    Y = rng.random((m, f))
    degrees = [4, 0, 3, 15, 1, 2]
    indptr = np.concatenate([[0], np.cumsum(degrees)]).astype(np.int64)
    indices = np.concatenate([rng.choice(m, d, replace=False) for d in degrees]).astype(np.int32)
    values = 10 * np.log1p(rng.integers(1, 6, len(indices)).astype(np.float64))
    values[2] = 0.0                                                # a stored zero
    indices[indptr[2] + 1] = indices[indptr[2]]                    # a duplicate: a separate entry
    targets = rng.integers(0, m, (len(degrees), 5)).astype(np.int32)
    targets[:, 0] = [indices[indptr[u]] if degrees[u] else 0 for u in range(len(degrees))]
    targets[1, 3] = targets[4, 1] = -1
    return Y, indptr, indices, values, targets


@pytest.mark.parametrize("bias", [0, 1])
def test_total_is_predict_on_the_folded_in_row(bias):
    Y, indptr, indices, values, targets = _small_case(bias, 11 + bias)
    assert indptr[2] == indptr[1] and 0.0 in values and indptr[4] - indptr[3] > Y.shape[1]
    lam = 0.3
    C = sp.csr_matrix((values, indices, indptr), shape=(len(indptr) - 1, len(Y)))
    assert C.nnz == len(values)                                    # as stored: the duplicate is not merged
    X = (orc.recompute_factors_bias if bias else orc.recompute_factors)(Y, C, lam, dtype="float64")
    contrib, total = ref.ref64(Y, bias, lam, indptr, indices, values, targets)
    for u in range(len(X)):
        ok = targets[u] >= 0
        want = orc.predict(X, Y, np.full(ok.sum(), u), targets[u][ok], bias=bool(bias))
        assert np.abs(total[u, ok] - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
        assert (total[u, ~ok] == 0).all() and (contrib[indptr[u]:indptr[u + 1]][:, ~ok] == 0).all()
    # the whitened form of the same numbers, in float64: q = y~ W_white, (I + sum w q q^T)^-1
    Yt, beta = ref.tilde(Y, bias)
    W = ref.whitening(Y, bias, lam)
    assert np.abs(W.T @ (Yt.T @ Yt + lam * np.eye(Y.shape[1])) @ W - np.eye(Y.shape[1])).max() <= 1e-12
    for u in (0, 3):
        j = indices[indptr[u]:indptr[u + 1]]
        w = values[indptr[u]:indptr[u + 1]] - beta[j]
        Q, qi = Yt[j] @ W, Yt[targets[u][targets[u] >= 0]] @ W
        white = (w + 1)[:, None] * (Q @ np.linalg.solve(np.eye(Y.shape[1]) + Q.T @ (Q * w[:, None]), qi.T))
        assert np.abs(white - contrib[indptr[u]:indptr[u + 1]][:, targets[u] >= 0]).max() <= 1e-12


@pytest.mark.parametrize("bias", [0, 1])
def test_golden_half_step(bias):
    """users1 of the fixture is the reference's own half step on items0: the totals are its scores.  The fixture's rows are
    float32 results, equal to the oracle's within RTOL / ATOL of tests/test_oracle_golden.py per factor, which bounds a score by
    sum_c (ATOL + RTOL |x_c|) |y~_c|."""
    g = load_golden(f"half_bias{bias}_float32.npz")
    C = csr_from(g, "C")
    Y, X, lam = g["items0"], g["users1"].astype(np.float64), float(g["gamma"])
    rng = np.random.default_rng(2)
    users = np.concatenate([[3], rng.choice(C.shape[0], 40, replace=False)])        # row 3 of the fixture is empty
    targets = rng.integers(0, len(Y), (len(users), 4)).astype(np.int32)
    lens = np.diff(C.indptr)[users]
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    pos = np.concatenate([np.arange(C.indptr[u], C.indptr[u + 1]) for u in users]).astype(np.int64)
    contrib, total = ref.ref64(Y, bias, lam, indptr, C.indices[pos], C.data[pos], targets)
    Yt, _ = ref.tilde(Y, bias)
    for k, u in enumerate(users):
        want = orc.predict(X, Y.astype(np.float64), np.full(4, u), targets[k], bias=bool(bias))
        bound = ((2e-6 + 2e-5 * np.abs(X[u]))[None, :] * np.abs(Yt[targets[k]])).sum(axis=1)
        if not bias and lens[k] == 0:
            assert (total[k] == 0).all()
        assert (np.abs(total[k] - want) <= bound).all(), (u, np.abs(total[k] - want).max(), bound.min())


def test_restatement_matches_the_definition_on_small_rows():
    """The float32 restatement against float64 where nothing is ill-conditioned, and its failure report."""
    c = ref.case("gauss_f16_b0")
    assert c["restated_err"].max() <= RESTATED_CAP["gauss"]
    f = 4
    Y = np.eye(6, f, dtype=np.float32)
    indptr, indices = np.array([0, 2, 3]), np.array([0, 1, 2], dtype=np.int32)
    values = np.array([3.0, -2.0, 3.0], dtype=np.float32)
    got, total = ref.restated32(Y, 0, np.eye(f, dtype=np.float32), indptr, indices, values, np.array([[0, -1], [2, 3]], dtype=np.int32))
    assert np.isnan(got[:2, 0]).all() and (got[:2, 1] == 0).all() and np.isnan(total[0, 0]) and total[0, 1] == 0
    assert got[2, 0] == 1.0 and got[2, 1] == 0 and total[1, 0] == 1.0      # (3 + 1) (1 / (1 + 3))


@pytest.mark.parametrize("name", ref.case_names())
def test_every_gpu_gate_is_capped(name):
    c = ref.case(name)
    cap = RESTATED_CAP[name.split("_")[0]]
    live = c["targets"] >= 0
    assert live.any() and len(c["indices"]) > 0
    assert np.isfinite(c["ref"]).all() and c["restated_err"][live].max() <= cap, (name, c["restated_err"][live].max())
    assert c["gate"][live].max() <= ref.GATE_MARGIN * cap + ref.GATE_FLOOR
    print(f"{name}: restated32 pair error {c['restated_err'][live].max():.3e}, cap {cap:.1e}")


def test_case_families_are_complete():
    names = ref.case_names()
    assert len(names) == len(set(names))
    for family in tuple(RESTATED_CAP):
        assert any(n.split("_")[0] == family for n in names), family
    widths = {(c["f"], c["ld"], c["bias"]) for c in map(ref.case, [n for n in names if n.startswith("width")])}
    for f in ref.WIDTHS:
        assert (f, ref.ld_for(f), 0) in widths and (f < 2 or (f, ref.ld_for(f), 1) in widths)
    for f, extra in ref.LD_EXTRA.items():
        assert (f, ref.ld_for(f, extra), 0) in widths and (f, ref.ld_for(f, extra), 1) in widths
    degrees = set(np.diff(ref.case("width_f65_b1_x0")["indptr"]).tolist())
    assert {0, 1, 2, 3, ref.CHUNK - 1, ref.CHUNK, ref.CHUNK + 1, 64, 65, 66} <= degrees
    assert 9000 in np.diff(ref.case("long_row")["indptr"]) and len(ref.case("grid_cap")["indptr"]) - 1 > ref.GRID_CAP
    assert sorted(ref.case(f"targets_T{T}")["targets"].shape[1] for T in ref.T_CYCLE) == [1, 2, ref.MAX_TARGETS - 1, ref.MAX_TARGETS]
    c = ref.case("neg_f65_b1")
    w = c["values"] - c["Y"][c["indices"], 0]
    assert (w > -1).all() and (w < 0).all()
    c = ref.case("eqbias_f129_b1")
    assert (c["values"] == c["Y"][c["indices"], 0]).any()
    assert (ref.case("zeros_f16_b0")["values"] == 0).any() and (ref.case("w1e3_f260_b0")["values"] > 900).any()
    c = ref.case("dup_f16_b0")
    assert c["indices"][c["indptr"][2]] == c["indices"][c["indptr"][2] + 1]


def test_orthogonal_closed_form():
    c, exact = ref.orthogonal_case()
    contrib, _ = ref.ref64(c["Y"][:, :c["f"]], 0, c["lam"], c["indptr"], c["indices"], c["values"], c["targets"])
    assert len(exact) > 20
    for (e, t), v in exact.items():
        assert abs(contrib[e, t] - float(v)) <= 1e-6 * abs(float(v))          # (W32 is W_white rounded to float32)
    bound, measured = ref.orthogonal_ulp_bound()
    print(f"orthogonal catalogue: restated32 is within {measured:.3f} ulp of the closed form; the device is held to {bound:.3f}")
    assert 0.5 <= measured <= 8.0


# ------------------------------------------------------------------------------------------------------- argument checks
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build()
    from recmodel_amd import _lib
    return _lib.load()


def test_entry_point_checks_its_arguments(lib):
    from recmodel_amd import _lib
    d = ctypes.c_void_p(16)
    need = lib.wmf_explain_workspace_bytes(10, 16, 4)
    assert need >= 1
    call = lambda **kw: lib.wmf_explain_rows(*[kw.get(k, v) for k, v in (  # noqa: E731
        ("Y", d), ("m", 100), ("f", 16), ("ld", 16), ("bias", 0), ("W", d), ("indptr", d), ("indices", d), ("values", d), ("n", 10),
        ("targets", d), ("T", 4), ("contrib", d), ("total", d), ("fail", d), ("ws", d), ("ws_bytes", 1 << 30), ("stream", None))])
    for bad in (dict(f=0), dict(f=261), dict(ld=15), dict(ld=12), dict(ld=276, f=260), dict(m=0), dict(m=1 << 31), dict(n=-1), dict(T=0),
                dict(T=17), dict(ws_bytes=need - 1), dict(Y=None), dict(W=None), dict(indptr=None), dict(indices=None), dict(values=None),
                dict(targets=None), dict(contrib=None), dict(total=None), dict(fail=None), dict(ws=None)):
        assert call(**bad) == _lib.WMF_EINVAL, bad
    assert b"n_targets" in (call(T=17), lib.wmf_last_error())[1]
    assert call(n=0) == _lib.WMF_OK                                # no rows: nothing is launched


def test_model_method_checks_its_arguments_before_the_gpu(monkeypatch):
    from recmodel_amd import WMF, _lib

    def touched():
        raise AssertionError("the GPU was asked for before the arguments were checked")
    monkeypatch.setattr(_lib, "require_gpu", touched)
    C = sp.random(6, 5, density=0.5, format="csr", random_state=0)
    m = WMF(num_items=5, num_users=6, dim=2, gamma=0.1, weighted=False)
    m.users = np.zeros((6, 2), dtype=np.float32)
    with pytest.raises(ValueError):
        m.explain([0], [[1]], C)
    m = WMF(num_items=5, num_users=6, dim=2, gamma=0.1, weighted=True)
    with pytest.raises(ValueError):
        m.explain([0], [[1]], C)                                   # no user factors yet
    m.users = np.zeros((6, 2), dtype=np.float32)
    for args, kw in ((([0], [[1]], sp.random(5, 6, density=0.5, format="csr", random_state=0)), {}),
                     (([0], [[1]], C.toarray()), {}),
                     (([0], [[1]], C), dict(pre_process_count="sqrt")),
                     (([0], [[1]], C), dict(topk=0)),
                     (([0, 1], [[1]], C), {}),                     # one row of items for two users
                     (([0, 1], [1, 2, 3], C), {}),
                     (([0], [[5]], C), {}),                        # an item id past the catalogue
                     (([0], [[-2]], C), {}),
                     (([0], [[0.5]], C), {}),
                     (([0], [[]], C), {}),
                     ((0, [[1, 2], [3, 4]], C), {})):              # an int user takes one list of items
        with pytest.raises(ValueError):
            m.explain(*args, **kw)
    with pytest.raises(IndexError):
        m.explain([6], [[1]], C)
    with pytest.raises(AssertionError):
        m.explain([0, -1], [[1, -1], [2, 3]], C)                   # well-formed: the next thing it does is ask for the GPU
