"""Folding histories in without a GPU: tests/foldin_ref.py against the oracle's recompute_factors[_bias] and the reference's own
goldens, the float32 restatement against the definition, the caps that keep every GPU gate meaningful, and the argument checks
of wmf_foldin_rows, WMF.fold_in and WMF.recommend_for."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import foldin_ref as ref
from conftest import csr_from, load_golden
from oracle import wmf_oracle as orc

# The largest row error the float32 restatement may have against float64 on the inputs of a family: 1.5 x the largest figure
# measured on the CPU for the committed cases (width 9.6e-6, gauss 2.2e-6, w1e3 1.7e-4, zeros 5.5e-6, dup 7.7e-6, eqbias 6.1e-6,
# neg 2.2e-6, long 4.7e-6, grid 1.2e-6).  A gate is 4 x the row's figure + 8 ulps, so no gate exceeds 4 x cap + 8 ulps: none is
# vacuous.
RESTATED_CAP = {"width": 1.4e-5, "gauss": 3.3e-6, "w1e3": 2.5e-4, "zeros": 8.2e-6, "dup": 1.1e-5, "eqbias": 9.2e-6, "neg": 3.3e-6,
                "long": 7.0e-6, "grid": 1.7e-6}


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
    return Y, indptr, indices, values


@pytest.mark.parametrize("bias", [0, 1])
def test_ref64_is_the_oracles_half_step(bias):
    Y, indptr, indices, values = _small_case(bias, 21 + bias)
    assert indptr[2] == indptr[1] and 0.0 in values and indptr[4] - indptr[3] > Y.shape[1]
    lam = 0.3
    C = sp.csr_matrix((values, indices, indptr), shape=(len(indptr) - 1, len(Y)))
    assert C.nnz == len(values)                                    # as stored: the duplicate is not merged
    want = (orc.recompute_factors_bias if bias else orc.recompute_factors)(Y, C, lam, dtype="float64")
    got = ref.ref64(Y, bias, lam, indptr, indices, values)
    assert got.shape == want.shape and (got[1] == 0).all()
    assert np.abs(got - want).max() <= 1e-10 * max(1.0, np.abs(want).max())
    # row by row through solve_row, and the whitened form of the same numbers in float64: x = W (I + E)^-1 W^T b
    Yt, beta = ref.tilde(Y, bias)
    G = orc.gramian(Yt, lam, "float64")
    W = ref.whitening(Y, bias, lam)
    for u in (0, 3, 5):
        j = indices[indptr[u]:indptr[u + 1]]
        w = values[indptr[u]:indptr[u + 1]] - beta[j]
        assert np.abs(got[u] - orc.solve_row(G, Yt, j, w)).max() <= 1e-10
        Q = Yt[j] @ W
        white = W @ np.linalg.solve(np.eye(Y.shape[1]) + Q.T @ (Q * w[:, None]), (w + 1) @ Q)
        assert np.abs(white - got[u]).max() <= 1e-10


@pytest.mark.parametrize("bias", [0, 1])
def test_golden_half_step(bias):
    """users1 of the fixture is the reference's own half step on items0, every row of it against every item, at the tolerance
    of test_explain_cpu.py::test_golden_half_step: the fixture's rows are float32 results, equal to the oracle's within RTOL /
    ATOL of tests/test_oracle_golden.py per factor, which bounds a score y~_i . x by sum_c (ATOL + RTOL |x_c|) |y~_c|."""
    g = load_golden(f"half_bias{bias}_float32.npz")
    C = csr_from(g, "C")
    Y, X, lam = g["items0"], g["users1"].astype(np.float64), float(g["gamma"])
    got = ref.ref64(Y, bias, lam, C.indptr.astype(np.int64), C.indices, C.data)
    assert got.shape == X.shape and (np.diff(C.indptr) == 0).any()
    Yt, _ = ref.tilde(Y, bias)
    bound = (2e-6 + 2e-5 * np.abs(X)) @ np.abs(Yt).T               # [rows, items]
    diff = np.abs((got - X) @ Yt.T)
    assert (diff <= bound).all(), (diff.max(), bound.min())
    if not bias:
        assert (got[np.diff(C.indptr) == 0] == 0).all()


def test_restatement_matches_the_definition_on_small_rows():
    """The float32 restatement against float64 where nothing is ill-conditioned, an empty row, and its failure report."""
    c = ref.case("gauss_f16_b0")
    assert c["restated_err"].max() <= RESTATED_CAP["gauss"]
    f = 4
    Y = np.eye(6, f, dtype=np.float32)
    indptr, indices = np.array([0, 2, 2, 3]), np.array([0, 1, 2], dtype=np.int32)
    values = np.array([3.0, -2.0, 3.0], dtype=np.float32)
    got = ref.restated32(Y, 0, np.eye(f, dtype=np.float32), indptr, indices, values)
    assert np.isnan(got[0]).all() and (got[1] == 0).all()
    assert np.array_equal(got[2], np.array([0, 0, 1, 0], dtype=np.float32))         # (3 + 1) / (1 + 3) on axis 2
    assert np.isinf(ref.row_errors(got, np.zeros((3, f)))[0])


@pytest.mark.parametrize("name", ref.case_names())
def test_every_gpu_gate_is_capped(name):
    c = ref.case(name)
    cap = RESTATED_CAP[name.split("_")[0]]
    live = c["live"]
    assert live.any() and np.isfinite(c["ref"]).all() and (c["ref"][~live] == 0).all()
    assert c["restated_err"][live].max() <= cap, (name, c["restated_err"][live].max())
    assert (c["restated_err"][~live] == 0).all() and c["gate"].max() <= ref.GATE_MARGIN * cap + ref.GATE_FLOOR
    print(f"{name}: restated32 row error {c['restated_err'][live].max():.3e}, cap {cap:.1e}")


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
    for f in (30, 31, 32):
        assert (f, ref.ld_for(f), 0) in widths and (f, ref.ld_for(f), 1) in widths
    degrees = np.diff(ref.case("width_f65_b1_x0")["indptr"]).tolist()
    assert {0, 1, 2, 3, ref.CHUNK - 1, ref.CHUNK, ref.CHUNK + 1, 64, 65, 66} <= set(degrees)
    assert degrees[0] == 0 and degrees[-1] == 0 and 0 in degrees[1:-1]               # empty rows first, in the middle, last
    for fam in ref.FAMILIES:
        for f, b in ref.FAMILY_WIDTHS:
            assert f"{fam}_f{f}_b{b}" in names
    assert 9000 in np.diff(ref.case("long_row")["indptr"]) and len(ref.case("grid_cap")["indptr"]) - 1 == 1030 > ref.GRID_CAP
    c = ref.case("neg_f65_b1")
    w = c["values"] - c["Y"][c["indices"], 0]
    assert (w > -1).all() and (w < 0).all()
    c = ref.case("eqbias_f129_b1")
    assert (c["values"] == c["Y"][c["indices"], 0]).any()
    assert (ref.case("zeros_f16_b0")["values"] == 0).any() and (ref.case("w1e3_f260_b0")["values"] > 900).any()
    c = ref.case("dup_f16_b0")
    assert c["indices"][c["indptr"][2]] == c["indices"][c["indptr"][2] + 1]


def test_orthogonal_closed_form():
    c, exact = ref.orthogonal_exact()
    X = ref.ref64(c["Y"][:, :c["f"]], 0, c["lam"], c["indptr"], c["indices"], c["values"])
    assert len(exact) > 20
    for u in range(len(X)):
        for a in range(c["f"]):
            if (u, a) in exact:
                assert abs(X[u, a] - float(exact[(u, a)])) <= 1e-6 * abs(float(exact[(u, a)]))   # (W32 is W_white rounded to float32)
            else:
                assert abs(X[u, a]) <= 1e-12
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
    need = lib.wmf_foldin_workspace_bytes(10, 16)
    assert need >= 1
    call = lambda **kw: lib.wmf_foldin_rows(*[kw.get(k, v) for k, v in (  # noqa: E731
        ("Y", d), ("m", 100), ("f", 16), ("ld", 16), ("bias", 0), ("W", d), ("indptr", d), ("indices", d), ("values", d), ("n", 10),
        ("X", d), ("fail", d), ("ws", d), ("ws_bytes", 1 << 30), ("stream", None))])
    for bad in (dict(f=0), dict(f=261), dict(ld=15), dict(ld=12), dict(ld=276, f=260), dict(m=0), dict(m=1 << 31), dict(n=-1),
                dict(n=1 << 31), dict(ws_bytes=need - 1), dict(Y=None), dict(W=None), dict(indptr=None), dict(indices=None),
                dict(values=None), dict(X=None), dict(fail=None), dict(ws=None)):
        assert call(**bad) == _lib.WMF_EINVAL, bad
    assert b"workspace" in (call(ws_bytes=0), lib.wmf_last_error())[1]
    assert call(n=0) == _lib.WMF_OK                                # no rows: nothing is launched


def test_model_methods_check_their_arguments_before_the_gpu(monkeypatch):
    from recmodel_amd import WMF, _lib, wmf_model

    def touched():
        raise AssertionError("the GPU was asked for before the arguments were checked")
    monkeypatch.setattr(_lib, "require_gpu", touched)
    C = sp.random(4, 5, density=0.5, format="csr", random_state=0)
    m = WMF(num_items=5, num_users=6, dim=2, gamma=0.1, weighted=False)
    m.users = np.zeros((6, 2), dtype=np.float32)
    for method in (m.fold_in, m.recommend_for):
        with pytest.raises(ValueError):
            method(C)                                              # not the weighted branch
    m = WMF(num_items=5, num_users=6, dim=2, gamma=0.1, weighted=True)
    m.users = np.zeros((6, 2), dtype=np.float32)
    items, m.items = m.items, None
    for method in (m.fold_in, m.recommend_for):
        with pytest.raises(ValueError):
            method(C)                                              # no item factors
    m.items = items
    for method in (m.fold_in, m.recommend_for):
        for args, kw in (((sp.random(4, 6, density=0.5, format="csr", random_state=0),), {}),      # 6 items, the model has 5
                         ((C.toarray(),), {}),
                         (([[0, 1, 0, 0, 2]],), {}),
                         ((C,), dict(pre_process_count="sqrt"))):
            with pytest.raises(ValueError):
                method(*args, **kw)
        with pytest.raises(AssertionError):
            method(C)                                              # well-formed, B != num_users: the next thing it does is ask for the GPU
        with pytest.raises(AssertionError):
            method(C.tocoo())
    for topn in (0, -1, wmf_model.RECOMMEND_MAX_TOPN + 1):
        with pytest.raises(ValueError):
            m.recommend_for(C, topn=topn)
    with pytest.raises(AssertionError):
        m.recommend_for(C, topn=wmf_model.RECOMMEND_MAX_TOPN)
