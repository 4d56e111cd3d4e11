"""AlsEngine.audit, WMF.objective / row_backward_errors and train(track_objective=True) on the GPU, against tests/audit_ref.py.

The matrix has 260 x 400 entries' worth of rows whose degrees hit every bin of wmf_plan_stats -- at most 8 entries (two rows per
wave), 9 .. 16, 17 .. 32, 33 .. 4096 (one wave or four per row; the iteration's candidates among them) and above 4096 (split into
segments) -- with duplicate columns, which is how 4500 entries fit into 400 items.  Widths: k = 16, 64, 128 + bias in rolled and
in plain coordinates, 208 + bias, 256.

What is compared with what:
  * `stored` (S1 - S2) and `n_stored` come from the float64 kernel alone: 1e-10 relative (tests/test_gpu_audit.py derives it).
  * `all_pairs`, `reg` and the dense term of eta go through wmf_gram, a float32 product.  tests/test_gpu_dense.py holds its
    column-scaled error max |dG_ij| / sqrt(G_ii G_jj) to at most that of NumPy's float32 product of the same operands, so this
    file measures that number e (for both Gramians, next to the comparison) and allows
        |d all_pairs| <= (e_X + e_Y) sum_ij sqrt(GX_ii GX_jj GY_ii GY_jj),   |d reg| <= e_X lambda tr GX,
        |d eta_u|     <= e_Y tr(G~) / |G~ + lambda I|_F        (|dG x| / ((|A| + a)|x| + |b|) <= |dG|_F / |A|_F),
    each doubled for the second-order terms.
  * The eta gates are measured, not derived: max eta per family of rows and width, next to the eta of np.linalg.solve in float32 on
    the same rows, in profiles/r10_audit_errors.json; a test allows 3 x the device's figure (the project's rule) and reads the file."""
import functools
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import audit_ref
from conftest import ROOT, record_error

pytestmark = pytest.mark.gpu

N_USERS, N_ITEMS, GAMMA = 260, 400, 0.1
DEGREES = (0, 1, 3, 8, 9, 16, 17, 32, 33, 40, 100, 600, 4096, 4097, 4500)
CASES = [(16, 0, None), (64, 0, None), (128, 1, True), (128, 1, False), (208, 1, None), (256, 0, None)]
FAMILIES = (("pairs", 1, 8), ("low16", 9, 16), ("low32", 17, 32), ("wave", 33, 4096), ("split", 4097, 1 << 40))
ERRORS_FILE = os.path.join(ROOT, "profiles", "r10_audit_errors.json")


def case_id(k, bias, rolled):
    return f"k{k}_b{bias}" + ("" if rolled is None else ("_rolled" if rolled else "_plain"))


case = pytest.mark.parametrize("k,bias,rolled", CASES, ids=[case_id(*c) for c in CASES])


@functools.lru_cache(maxsize=None)
def matrix():
    """(counts CSR as stored -- duplicates kept --, its transpose, both float32 with integer counts 1 .. 5)."""
    rng = np.random.default_rng(2024)
    deg = np.concatenate([DEGREES, rng.poisson(20, N_USERS - len(DEGREES) - 1), [0]]).astype(np.int64)
    indptr = np.concatenate([[0], np.cumsum(deg)])
    indices = np.concatenate([np.sort(rng.integers(0, N_ITEMS, d)) for d in deg]).astype(np.int32)
    data = rng.integers(1, 6, int(indptr[-1])).astype(np.float32)
    C = sp.csr_matrix((data, indices, indptr), shape=(N_USERS, N_ITEMS))
    CT = C.T.tocsr()
    assert C.nnz == CT.nnz == int(indptr[-1]) and not C.has_canonical_format        # duplicates survive, in both orientations
    return C, CT


def confidence(mat, mode="log"):
    out = sp.csr_matrix((audit_ref.confidence(mat.data.astype(np.float32), 10, 1, mode).astype(np.float32), mat.indices, mat.indptr),
                        shape=mat.shape)
    return out


def family_of(deg):
    return [name for name, lo, hi in FAMILIES if lo <= deg <= hi][0] if deg else None


def gate(key):
    table = json.load(open(ERRORS_FILE))["audit_eta"] if os.path.exists(ERRORS_FILE) else {}
    assert key in table, f"{key}: no measured eta in profiles/r10_audit_errors.json"
    return 3.0 * table[key]


def scaled_gram_error(Y, bias):
    """max |dG_ij| / sqrt(G_ii G_jj) of NumPy's float32 product y~^T y~ against the float64 one."""
    Yt = audit_ref.y_tilde(Y, bias)
    G = Yt.T @ Yt
    G32 = (Yt.astype(np.float32).T @ Yt.astype(np.float32)).astype(np.float64)
    d = np.sqrt(np.diag(G))
    return float(np.max(np.abs(G32 - G) / np.outer(d, d))), G


def tolerances(X, Y, bias):
    """(|d all_pairs|, |d reg|, |d eta|) allowed for wmf_gram's float32 products (module docstring)."""
    eX, GX = scaled_gram_error(X, False)
    eY, GY = scaled_gram_error(Y, bias)
    dX, dY = np.sqrt(np.diag(GX)), np.sqrt(np.diag(GY))
    A = GY + GAMMA * np.eye(len(GY))
    return (2 * (eX + eY) * float(np.sum(np.outer(dX, dX) * np.outer(dY, dY))), 2 * eX * GAMMA * float(np.trace(GX)),
            2 * eY * float(np.trace(GY)) / float(np.linalg.norm(A)))


def numpy_float32_rows(Y, bias, M):
    """The rows np.linalg.solve gives in float32 on the same systems (wmf_model.py:237-239 / :343-350 on float32 inputs)."""
    Y = np.asarray(Y, dtype=np.float32)
    Yt = Y.copy()
    beta = Y[:, 0].copy() if bias else np.zeros(len(Y), dtype=np.float32)
    if bias:
        Yt[:, 0] = 1.0
    f = Y.shape[1]
    A0 = Yt.T @ Yt + np.float32(GAMMA) * np.eye(f, dtype=np.float32)
    X = np.zeros((M.shape[0], f), dtype=np.float32)
    for u in range(M.shape[0]):
        lo, hi = M.indptr[u], M.indptr[u + 1]
        if hi == lo:
            continue
        Yu = Yt[M.indices[lo:hi]]
        w = M.data[lo:hi].astype(np.float32) - beta[M.indices[lo:hi]]
        X[u] = np.linalg.solve(A0 + Yu.T @ (Yu * w[:, None]), (w + 1) @ Yu)
    return X


def new_engine(k, bias, rolled, monkeypatch):
    from recmodel_amd.engine import AlsEngine
    if rolled is not None:
        monkeypatch.setenv("WMF_ROLLED", "1" if rolled else "0")
    eng = AlsEngine(N_USERS, N_ITEMS, k, bool(bias), GAMMA)
    assert rolled is None or eng.rolled == rolled
    W = confidence(matrix()[0])
    eng.set_interactions(torch.from_numpy(W.indptr.astype(np.int64)), torch.from_numpy(W.indices.astype(np.int64)), torch.from_numpy(W.data))
    users = eng.csr["users"]
    assert users.bin_rows[0] > 0 and users.bin_rows[1] > 0 and users.bin_rows[2] + users.bin_rows[3] > 0      # every bin of the plan
    assert users.rows8 > 0 and users.rows_split > 0
    rng = np.random.default_rng(k + bias)
    f = k + bias
    eng.set_factors("users", rng.random((N_USERS, f)).astype(np.float32))
    eng.set_factors("items", rng.random((N_ITEMS, f)).astype(np.float32))
    return eng


def check_against_reference(got, X, Y, bias, M, eta=None):
    want = audit_ref.audit(X, Y, bool(bias), GAMMA, M.indptr, M.indices, M.data, rows=eta is not None)
    t_pairs, t_reg, t_eta = tolerances(X, Y, bool(bias))
    scale = abs(want["all_pairs"]) + abs(want["stored"]) + want["reg"]
    assert got["n_stored"] == want["n_stored"] == M.nnz
    assert abs(got["stored"] - want["stored"]) <= 1e-10 * scale, (got["stored"], want["stored"])
    assert abs(got["all_pairs"] - want["all_pairs"]) <= t_pairs, (got["all_pairs"], want["all_pairs"], t_pairs)
    assert abs(got["reg"] - want["reg"]) <= t_reg, (got["reg"], want["reg"], t_reg)
    assert abs(got["loss"] - want["loss"]) <= t_pairs + t_reg + 1e-10 * scale
    if eta is not None:
        assert np.max(np.abs(eta - want["eta"])) <= t_eta, (np.max(np.abs(eta - want["eta"])), t_eta)
    return want


@case
def test_half_step_lowers_the_objective_and_solves_every_row(k, bias, rolled, monkeypatch):
    from oracle import wmf_oracle as orc
    eng = new_engine(k, bias, rolled, monkeypatch)
    C, CT = (confidence(m) for m in matrix())
    name = case_id(k, bias, rolled)
    step = orc.recompute_factors_bias if bias else orc.recompute_factors
    measured, deg_all = {}, {}
    for side, other, M in (("users", "items", C), ("items", "users", CT)):
        before = eng.audit(side)["loss"]
        eng.half_step(side)
        eng.check_numerics()
        got = eng.audit(side, rows=True)
        eta = got.pop("eta").cpu().numpy()
        assert got["loss"] <= before, (side, got["loss"], before)
        X, Y = eng.get_factors(side), eng.get_factors(other)
        want = check_against_reference(got, X, Y, bias, M, eta)
        scale = abs(want["all_pairs"]) + abs(want["stored"]) + want["reg"]
        # the objective at the float64 oracle's solution of the same half step (float64 Gramian too): the minimum itself
        M64 = sp.csr_matrix((M.data.astype(np.float64), M.indices, M.indptr), shape=M.shape)
        best = audit_ref.audit(step(Y.astype(np.float64), M64, GAMMA, dtype="float64", out_dtype="float64"), Y, bool(bias), GAMMA, M.indptr, M.indices,
                               M.data)["loss"]
        assert want["loss"] >= best - 1e-12 * scale                # nothing lies below the minimum (1e-12: the sums' own rounding)
        measured[f"{name}_{side}_margin"] = abs(got["loss"] - best) / scale
        # eta per family of rows, next to NumPy's float32 solve of the same rows
        eta_np = audit_ref.audit(numpy_float32_rows(Y, bias, M), Y, bool(bias), GAMMA, M.indptr, M.indices, M.data, rows=True)["eta"]
        deg = np.diff(M.indptr)
        fam = np.array([family_of(d) for d in deg], dtype=object)
        for family in sorted({x for x in fam if x}):
            rows = fam == family
            measured[f"{name}_{side}_{family}"] = float(eta[rows].max())
            measured[f"{name}_{side}_{family}_numpy"] = float(eta_np[rows].max())
        assert not eta[deg == 0].any()                             # an empty row: x = 0, b = 0
    print(json.dumps(measured, sort_keys=True))
    record_error("audit_eta", **measured)
    assert {key.split("_")[-1] for key in measured if "_users_" in key} >= {name for name, _, _ in FAMILIES}
    for key, value in measured.items():
        if not key.endswith("_numpy"):
            assert value <= gate(key), (key, value, gate(key))


@pytest.mark.parametrize("k,bias", [(64, 0), (128, 1)])
def test_a_scaled_row_stands_out(k, bias, monkeypatch):
    eng = new_engine(k, bias, None, monkeypatch)
    eng.half_step("users")
    eng.half_step("items")
    items = eng.get_factors("items")
    row = 7
    assert np.diff(matrix()[1].indptr)[row] > 0
    items[row] *= np.float32(1.01)
    eng.set_factors("items", items)
    eta = eng.audit("items", rows=True)["eta"].cpu().numpy()
    worst = max(gate(key) for key in json.load(open(ERRORS_FILE))["audit_eta"]
                if key.startswith(f"k{k}_b{bias}_") and "_items_" in key and not key.endswith(("_numpy", "_margin")))
    assert int(np.argmax(eta)) == row and eta[row] > worst, (row, int(np.argmax(eta)), eta[row], worst)


def test_train_tracks_an_objective_that_never_rises():
    from recmodel_amd import WMF
    C, CT = matrix()
    model = WMF(num_items=N_ITEMS, num_users=N_USERS, dim=32, gamma=GAMMA, weighted=True, bias=False)
    reg_items0 = GAMMA * float(np.sum(model.items.astype(np.float64) ** 2))
    plain = WMF(num_items=N_ITEMS, num_users=N_USERS, dim=32, gamma=GAMMA, weighted=True, bias=False)
    kw = dict(utility_mat=C, iterations=3, eval_mat=C, count_mat=C, cores=1, stopping_rounds=10, pre_process_count="linear", alpha=2)
    assert model.train(track_objective=True, **kw) == plain.train(**kw) == 2
    assert np.array_equal(model.users, plain.users) and np.array_equal(model.items, plain.items)     # tracking changes nothing
    assert not hasattr(plain, "objective_history")
    hist = model.objective_history
    assert [h["iteration"] for h in hist] == [0, 1, 2] and all(set(h) == {"iteration", "users", "items"} for h in hist)
    # L + gamma |F|^2: the fixed side's term is the `reg` of the half step before (the initial items' for the first)
    totals, reg_fixed = [], reg_items0
    for h in hist:
        for side in ("users", "items"):
            totals.append(h[side]["loss"] + reg_fixed)
            reg_fixed = h[side]["reg"]
    print("objective:", totals)
    assert all(b <= a for a, b in zip(totals, totals[1:])), totals
    assert totals[-1] < 0.9 * totals[0]
    # the public methods on the pulled factors ('linear' with alpha = 2 on integer counts: the float32 transform is exact)
    W, WT = (sp.csr_matrix((2.0 * m.data.astype(np.float64), m.indices, m.indptr), shape=m.shape) for m in (C, CT))
    for side, X, Y, M in (("users", model.users, model.items, W), ("items", model.items, model.users, WT)):
        got = model.objective(C, side=side, alpha=2, pre_process_count="linear")
        assert all(isinstance(got[key], float) for key in ("loss", "all_pairs", "stored", "reg")) and isinstance(got["n_stored"], int)
        eta = model.row_backward_errors(C, side=side, alpha=2, pre_process_count="linear")
        assert eta.dtype == np.float64 and eta.shape == (len(X),)
        check_against_reference(got, X, Y, 0, M, eta)
    assert abs(model.objective(C, side="items", alpha=2, pre_process_count="linear")["loss"] - hist[-1]["items"]["loss"]) <= 1e-12 * abs(totals[-1])


@pytest.mark.parametrize("k,bias", [(16, 0), (64, 1)])
def test_float64_path(k, bias):
    """cores = 2 on float64 counts keeps float64 factors: history and public methods come from the float64 entry point, and every
    row of the side solved last is at float64 roundoff."""
    from recmodel_amd import WMF
    C, CT = (sp.csr_matrix((m.data.astype(np.float64), m.indices, m.indptr), shape=m.shape) for m in matrix())
    model = WMF(num_items=N_ITEMS, num_users=N_USERS, dim=k, gamma=GAMMA, weighted=True, bias=bool(bias))
    model.train(utility_mat=C, iterations=2, eval_mat=C, count_mat=C, cores=2, stopping_rounds=10, track_objective=True)
    assert model.users.dtype == np.float64 and len(model.objective_history) == 2
    name = f"f64_k{k}_b{bias}"
    W, WT = (sp.csr_matrix((audit_ref.confidence(m.data), m.indices, m.indptr), shape=m.shape) for m in (C, CT))
    for side, X, Y, M in (("users", model.users, model.items, W), ("items", model.items, model.users, WT)):
        got = model.objective(C, side=side)
        eta = model.row_backward_errors(C, side=side)
        want = audit_ref.audit(X, Y, bool(bias), GAMMA, M.indptr, M.indices, M.data, rows=True)
        for key in ("loss", "all_pairs", "stored", "reg"):
            assert abs(got[key] - want[key]) <= 1e-10 * abs(want["loss"]), (side, key, got[key], want[key])
        assert got["n_stored"] == M.nnz and np.max(np.abs(eta - want["eta"])) <= 1e-12
    assert abs(got["loss"] - model.objective_history[-1]["items"]["loss"]) <= 1e-12 * abs(got["loss"])
    measured = {f"{name}_items": float(eta.max())}
    print(json.dumps(measured))
    record_error("audit_eta", **measured)
    assert eta.max() <= gate(f"{name}_items")
    if not bias:
        losses = [h[s]["loss"] for h in model.objective_history for s in ("users", "items")]
        assert losses[2] + model.objective_history[0]["items"]["reg"] <= losses[1] + model.objective_history[0]["users"]["reg"]
