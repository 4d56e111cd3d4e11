"""tests/iter_ref.py -- the reference tests/test_gpu_iter_rows.py is gated on -- checked without a GPU: solve_rows_ref against
oracle.solve_row on a whitened golden half step, its layouts against each other, route() / iter_dmax() against the widths the
routing tests pin, and, for EVERY case the GPU file builds, the margins that make policy()'s float64 prediction of a row's path
the float32 kernel's: the device evaluates the same tests in float32 (sums of up to 256 x 260 products: relative error below
1e-4), so a row whose every decision is a factor 1.1 and more away from its threshold takes the predicted path."""
import numpy as np
import pytest

import iter_ref as R
from conftest import load_golden
from oracle import wmf_oracle as orc


def _whitened_golden():
    g = load_golden("half_bias1_float32.npz")
    Y = g["items0"].astype(np.float64)
    bias = g["items0"][:, 0].copy()
    Yt = Y.copy()
    Yt[:, 0] = 1.0
    G = Yt.T @ Yt + float(g["gamma"]) * np.eye(Y.shape[1])
    L = np.linalg.cholesky(G)
    V = np.linalg.solve(L, Yt.T).T.astype(np.float32)                # V = Y~ L^-T
    return g, Yt, bias, G, L, V


def test_reference_against_the_oracle_on_a_whitened_golden_case():
    """x_u = g_u L^-1 (include/wmf_hip.h, W_unwhite) is the oracle's row; the whitened side is rounded to float32 before the
    reference sees it, which moves a row by cond(A_u) 6e-8 at the most."""
    g, Yt, bias, G, L, V = _whitened_golden()
    f = Yt.shape[1]
    assert R.is_split(f, 1) and R.ld_for(f) == 20
    indptr, indices, values = g["C_indptr"].astype(np.int64), g["C_indices"], g["C_data"]
    plain = np.zeros((V.shape[0], 20), dtype=np.float32)
    plain[:, :f] = V
    got_plain = R.solve_rows_ref(plain, None, bias, indptr, indices, values, f)
    side = np.stack([V[:, f - 1], bias], axis=1)
    got_split = R.solve_rows_ref(np.ascontiguousarray(V[:, :f - 1]), side, None, indptr, indices, values, f)
    assert np.array_equal(got_plain, got_split)                      # the two layouts hold the same numbers
    assert not got_plain[:, f:].any()
    worst, seen_empty = 0.0, False
    for u in range(len(indptr) - 1):
        idx = indices[indptr[u]: indptr[u + 1]]
        if not len(idx):
            assert not got_plain[u].any()
            seen_empty = True
            continue
        w = values[indptr[u]: indptr[u + 1]].astype(np.float64) - bias[idx]
        want = orc.solve_row(G, Yt, idx, w)
        x = np.linalg.solve(L.T, got_plain[u, :f])                   # x = L^-T g
        worst = max(worst, np.linalg.norm(x - want) / np.linalg.norm(want))
    assert worst <= 1e-5, worst
    f32 = R.solve_rows_f32(plain, None, bias, indptr, indices, values, f)
    assert f32.dtype == np.float32 and R.row_errors(f32, got_plain).max() <= 1e-4
    assert seen_empty or (np.diff(indptr) > 0).all()


def test_rolled_form_is_the_split_layout_with_the_bias_in_the_bits():
    case = R.build_case(129, 1, True)
    assert np.unique(case.side[:, 0]).size == 1
    assert np.array_equal(R.rolled_bias(case.V), case.side[:, 1])
    as_split = R.solve_rows_ref(case.V, case.side, None, case.indptr, case.indices, case.values, 129, rolled=False)
    assert np.array_equal(case.ref(), as_split)


def test_route_and_dmax_at_the_widths_the_routing_tests_pin():
    """tests/test_gpu_routing.py's ROUTES, read off the library: the iteration kernels of its cases are route()'s."""
    import test_gpu_routing as T
    for k, bias, rolled in T.CASES:
        names = {n for n in T.ROUTES[T.case_id(k, bias, rolled)] if n.startswith("solve_iter_kernel")}
        assert names == set(R.route(k + bias, bias, bool(rolled))), (k, bias, rolled)
    assert [f for f in range(1, 261) if R.is_split(f, 1)] == [17, 33, 65, 81, 97, 129] and not any(R.is_split(f, 0) for f in range(261))
    assert (R.iter_dmax(64, 0), R.iter_dmax(65, 0), R.iter_dmax(65, 1), R.iter_dmax(66, 1)) == (0, 144, 0, 144)
    assert (R.iter_dmax(128, 0), R.iter_dmax(129, 1), R.iter_dmax(129, 0), R.iter_dmax(256, 1), R.iter_dmax(257, 1)) == (128, 128, 256, 256, 192)
    assert {64, 65, 66, 80, 81, 82, 96, 97, 98, 124, 125, 127, 128, 129, 130, 188, 189, 192, 193, 252, 253, 256, 257, 260} <= set(R.WIDTHS)
    every = {n for f in range(1, 261) for b in (0, 1) for r in (False, True) for n in R.route(f, b, r)}
    main = {n for f, b, r in R.MAIN for n in R.route(f, b, r)}
    assert every == main, sorted(every - main)                       # one main width per shipped instantiation


def test_policy_on_rows_whose_path_is_known():
    """E = t u u^T (one entry, unit vector, weight t): the series is geometric at rate t, so the number of applications is the
    smallest k with t^(k + 1) <= eps (1 - 0); the Chebyshev start, the bounce on kappa and the bounce on tau_minus by hand."""
    u = np.zeros((1, 8))
    u[0, 0] = 1.0
    for t in (0.01, 0.05):                                           # (contraction t^2 per application, below max(sigma^2, 0.01): no switch)
        path, napp = R.policy(u, np.array([t]))
        want = next(k for k in range(1, 21) if t ** (k + 1) <= R.EPS)
        assert (path, napp) == ("neumann", want), (t, path, napp)
    assert R.policy(u, np.array([0.5]))[0] == "switch"               # rate 0.25 > sigma^2 = 0.01
    assert R.policy(u, np.array([0.5]), cheb=False) == ("handed_on", 1)
    assert R.policy(u, np.array([2.0]))[0] == "chebyshev"
    assert R.policy(u, np.array([2.0]), cheb=False) == ("handed_on", 0)
    assert R.policy(u, np.array([3.5])) == ("bounced", 0)            # chi = 4.5 > 4
    two = np.eye(2, 8)
    assert R.policy(two, np.array([0.3, -0.6])) == ("bounced", 0)    # tau = 0.9 > 0.8, tau_minus > 1/2
    assert R.policy(two, np.array([0.05, -0.7])) == ("bounced", R.KMAX)   # Neumann at rate 0.7: 0.7^21 > eps
    d = R.policy_detail(u, np.array([2.0]))
    assert abs(d["x"][0] - 1.0) <= 1e-6                              # (1 + 2)^-1 (2 + 1)


FAMILY_PATHS = {"A": {"neumann"}, "B": {"neumann"}, "C": {"switch"}, "D": {"chebyshev"}, "Da": {"chebyshev"}, "E": {"bounced"},
                "F": {"neumann"}, "G": {"bounced"}, "H": {"bounced"}}
FAMILY_APPS = {"A": (2, 3), "B": (4, 5), "D": (11, 14), "Da": (11, 14), "E": (0, 0), "G": (0, 0), "H": (R.KMAX, R.KMAX)}


def _check_case(case, name, families=True):
    final, stage1 = case.predict()
    bad = R.margins(case, final)
    assert not bad, (name, bad[:6])
    cond = R.conditions(case)
    assert cond.max() <= 100, (name, int(cond.argmax()), float(cond.max()))
    special = set(case.labels.values())
    for u in np.flatnonzero(case.candidate):
        fam, p = case.family[u], final[u]
        if families and u not in special:
            assert p["path"] in FAMILY_PATHS[fam], (name, u, fam, int(case.degree[u]), p["path"], p["applications"])
            if fam in FAMILY_APPS:
                lo, hi = FAMILY_APPS[fam]
                assert lo <= p["applications"] <= hi, (name, u, fam, int(case.degree[u]), p["applications"])
        if case.ldv == 128:
            want = {"neumann": "neumann"}.get(p["path"], "handed_on")
            assert stage1[u] == want, (name, u, fam, stage1[u], p["path"])
    if families and "H" in set(case.family):
        h = [final[u] for u in np.flatnonzero(case.candidate & (case.family == "H"))]
        assert all(p["tau_minus"] > 0.55 and 0.6 <= p["tau"] <= 0.8 for p in h)
    if families and "E" in set(case.family):
        e = [final[u] for u in np.flatnonzero(case.candidate & (case.family == "E"))]
        assert all(p["chi"] / p["alo"] > 4.4 for p in e)
    return final


@pytest.mark.parametrize("f,bias,rolled", R.MAIN, ids=[R.case_id(*c) for c in R.MAIN])
def test_main_cases_keep_their_margins(f, bias, rolled):
    case = R.build_case(f, bias, rolled)
    final = _check_case(case, R.case_id(f, bias, rolled))
    deg = set(case.degree[case.family == "A"].tolist())
    assert set(range(31, case.dmax + 3)) <= deg
    assert {"A", "B", "C", "D", "Da", "E", "F", "G", "H", ""} == set(case.family)
    assert {"stored_zero", "duplicate"} == set(case.labels)
    done, bounced, apps, cheb = case.expected_stats(final)
    assert done + bounced == int(case.candidate.sum()) and 0 < cheb < done and bounced > 0


def test_minor_cases_keep_their_margins():
    for f, bias in R.minor_cases():
        case = R.minor_case(f, bias)
        _check_case(case, R.case_id(f, bias, False))
        assert (case.degree == 0).any() and (case.degree > max(case.dmax, 33)).any()


@pytest.mark.parametrize("f,bias,rolled", R.MAIN, ids=[R.case_id(*c) for c in R.MAIN])
def test_pipeline_cases_keep_their_margins(f, bias, rolled):
    distinct, clones, which = R.pipeline_case(f, bias, rolled)
    final = _check_case(distinct, "pipeline-" + R.case_id(f, bias, rolled))
    assert clones.n == 4 * R.grid_cap(f, bias) + 37 and clones.n <= 16421 and set(which.tolist()) == set(range(32))
    assert distinct.candidate.all() and {33, distinct.dmax} <= set(distinct.degree.tolist())
    assert all(p["path"] in R.SOLVED for p in final)
    if distinct.ldv == 128:                                          # the whole list goes through the hand-over
        assert all(p["path"] == "switch" for p in final) and clones.degree.max() <= 128
    u = int(np.flatnonzero(which == 5)[-1])
    lo, hi = clones.indptr[u], clones.indptr[u + 1]
    assert np.array_equal(clones.indices[lo:hi], distinct.indices[distinct.indptr[5]: distinct.indptr[6]])
    one = R.single_row(distinct, 5)
    assert np.array_equal(one.ref()[0], distinct.ref()[5])
