"""The short-row kernels (csrc/wmf_solve.hip: solve_pair_kernel, solve_low_kernel, every NCH = 1 .. 17 with and without the split-f16
S tiles) and the two pivoted fallbacks PER ROW through wmf_plan_create / wmf_solve_rows_ex, against tests/low_ref.py: every degree
0 .. 33 at every width where the dispatch changes, on rows where every S entry matters.

The whitened side is an argument of wmf_solve_rows, so a case needs no half step: 600 hand-made rows, one block per family (norms
0.03, 0.3, 0.9, an aligned block, 1e-3 and 1e-4), weights from 1 to 1e6.  Every input sits between guard rows of NaN (an index guard
points into them), the output between sentinel rows; fail_count sits between poisoned neighbours.

Gates (a row's error is ||got - ref|| / ||ref|| against iter_ref.solve_rows_ref on exactly the uploaded float32 arrays):
    a row a short-row kernel solved   4 E_lr32 + T_x6.  E_lr32: the worst row error, over the row's (case, family, degree class), of
                                      the same d x d algorithm in NumPy float32 (for d >= 17 also of the symmetric form); T_x6: the
                                      row's distance from the reference when S is the split-f16 tile of the X6 kernels (0 elsewhere).
                                      tests/test_low_ref_cpu.py asserts that this is at most 2e-5 on every such row of every case.
                                      Margin 4 as in tests/test_gpu_iter_rows.py: lane and MFMA order against BLAS order.
    ... of 17 .. 32 entries that are  16.5 E_lr32 + T_x6 -- the aligned family, and every family at f <= 2.  On the device these rows
    nearly one direction              are 4 .. 9.3 x E_lr32 (12.8 at f = 1); the 2 x 2 block elimination restated in NumPy float32
                                      (low_ref.emulate_low) is 11 x E_lr32 on the host, so the margin is 1.5 x that figure.  Every other
                                      (family, class) restates below 4 (tests/test_low_ref_cpu.py).
    a bounced row                     22.8 E_lu32, E_lu32 the worst error of iter_ref.solve_rows_f32 (f x f, LAPACK) on the case's bounced rows.
                                      The pivoted kernels re-round the right-hand side in each of the f elimination steps where LAPACK
                                      subtracts one accumulated sum: restated (low_ref.emulate_pivoted) 6.5 x E_lu32 in the median and 15.2 at
                                      f = 258, measured 3 .. 4.3 up to f = 81, 12.6 at f <= 144 and 18.9 above; 1.5 x the restated figure.
    a row of 33 entries               tests/test_gpu_parity.py's 5e-4 (1e-3 above f = 144): another kernel family (its stiff and aligned rows are
                                      tamed on the f x f matrix those kernels eliminate)
    a row without entries             exactly 0; an exactly singular row: exactly 0 and counted in fail_count
In the launched-kernels test a (family, class) is ONE row, so E_lr32 is the worst of the float32 forms over four orders of the
features and of the entries (low_ref.yardsticks(orders=4)): one evaluation is no sample of what the order of the sums does to a row.

What this file found: gj_step normalised the pivot row in place, row_K += ((1 - piv) / piv) row_K, which rounds at 2^-24 of one and
not of 1 / piv -- a relative error of 6e-8 piv.  The stiff rows (w |v|^2 ~ 8e5) came back 0.1 % .. 13 % wrong from all three
templates (1e4 .. 5e5 x E_lr32), the balanced ones a few ulp.  The sweep now leaves pivot rows un-normalised and scales the
solution once, as gj_inv_step already did.
Measured on an MI355X after that fix (profiles/r15_low_rows.json), worst error / yardstick and worst row error per template:
    solve_pair_kernel      f32 tiles 3.5 (tiny), 3.6e-6 (stiff);   X6 2.8, 3.4e-7
    solve_low_kernel<1>    f32 tiles 3.3,        2.3e-6 (stiff);   X6 3.4, 8.8e-7
    solve_low_kernel<2>    f32 tiles 3.1,        3.0e-6 (stiff);   X6 2.7, 2.9e-6;  the aligned rows 8.2 / 9.3, 1.1e-6; f = 1: 12.8, 5.0e-6
    solve_general_kernel   12.6, 8.8e-7;  solve_wide_lu_kernel 18.9, 1.5e-6;  33 entries: 5.2e-4 (f > 144)
    at most 0.88 of a gate.  22 s for the file beside an MI355X, nearly all of it the host references."""
import numpy as np
import pytest
import torch

import low_ref as L
from conftest import record_error
from test_gpu_iter_rows import GUARD, SENTINEL, SOLVE_ROLLED, _Device, _guarded, _launches, _upload_rows  # noqa: F401

pytestmark = pytest.mark.gpu

CASE_IDS = [L.case_id(*c) for c in L.CASES]
LOW = ("solve_pair_kernel", "solve_low_kernel")
PIVOTED = ("solve_general_kernel", "solve_wide_lu_kernel")


def _solve(case, dev=None, profile=False, fails=0):
    """One wmf_solve_rows_ex over the case in a plan of its own, with the assertions of tests/test_gpu_iter_rows.py::_solve (nothing
    written outside, padding exactly 0, finite, fail_count between poisoned neighbours).  Returns (g [n, ld], kernel names)."""
    from recmodel_amd.engine import HipKernels
    K = HipKernels()
    dev = dev or _Device(case)
    ipd, (ixbuf, ix), (vbuf, vals) = _upload_rows(case)
    n, f, ld = case.n, case.f, case.ld
    gbuf = torch.full((n + 2 * GUARD, ld), SENTINEL, dtype=torch.float32, device="cuda")
    fail = torch.zeros(4, dtype=torch.int32, device="cuda")
    fail[1:] = 77
    plan, _ = K.plan_create(np.ascontiguousarray(case.indptr), n, f, case.bias)
    try:
        def run():
            K.solve_rows(plan, dev.V[1], dev.side[1], ipd, ix, vals, n, f, ld, gbuf[GUARD:], fail, flags=SOLVE_ROLLED if case.rolled else 0)
        names = _launches(K.lib, run)[1] if profile else run()
        torch.cuda.synchronize()
    finally:
        K.plan_destroy(plan)
    got = gbuf.cpu().numpy()
    assert np.all(got[:GUARD] == SENTINEL) and np.all(got[GUARD + n:] == SENTINEL), "a write outside the output rows"
    assert fail.tolist() == [fails, 77, 77, 77], fail.tolist()
    g = got[GUARD: GUARD + n]
    assert not (g == SENTINEL).any(), ("a sentinel survived", np.flatnonzero((g == SENTINEL).any(axis=1))[:8])
    assert np.isfinite(g).all(), ("a guard row was read", np.flatnonzero(~np.isfinite(g).all(axis=1))[:8])
    assert not g[:, f:].any(), "padding columns of g are not exactly 0"
    return g, names


_RUNS, _WORST = {}, {}


def _run_case(f, bias, rolled):
    key = (f, bias, rolled)
    if key not in _RUNS:
        _RUNS[key] = _solve(L.build_case(*key), profile=True)
    return _RUNS[key]


def _check_names(case, names):
    r = case.route
    assert {n for n in names if n.startswith(LOW)} == L.low_names(r), sorted(names)
    assert {n for n in names if n.startswith(PIVOTED)} == {r.fallback}, sorted(names)


def _gate_rows(name, case, g, orders=1, record=True):
    """Every row against its gate; records the worst error / yardstick per kernel template and family."""
    ref = case.ref()
    gate, kind, E, ys = L.gates(case, ref, orders=orders)
    err = L.row_errors(g, ref)
    exact = gate == 0
    assert not g[exact].any(), (name, "a row without entries (or an exactly singular one) is not exactly 0", np.flatnonzero(exact & g.any(axis=1))[:8])
    bad = [(int(u), kind[u], case.family[u], case.tags[u], int(case.degree[u]), float(err[u]), float(gate[u]))
           for u in np.flatnonzero(~exact) if not err[u] <= gate[u]]
    stats = {}
    x6 = "x6" if case.route.x6 else "f32"
    for (key, e) in E.items():
        if key == "bounced":
            sel = kind == "bounced"
            label, worst_key = "bounced", ("pivoted", case.route.fallback.split("<")[0], "negative")
        else:
            sel = (kind == key[1]) & (case.family == key[0])
            label, worst_key = f"{key[1]}.{key[0]}", (key[1], x6, key[0])
        stats[f"{label}.worst"], stats[f"{label}.yardstick"] = float(err[sel].max()), e
        stats[f"{label}.ratio"] = float(err[sel].max() / e) if e > 0 else 0.0
        stats[f"{label}.worst_over_gate"] = float((err[sel] / gate[sel]).max())
        w = _WORST.setdefault(".".join(worst_key), {"ratio": 0.0, "worst": 0.0, "worst_over_gate": 0.0})
        w["ratio"] = max(w["ratio"], stats[f"{label}.ratio"])
        w["worst"] = max(w["worst"], stats[f"{label}.worst"])
        w["worst_over_gate"] = max(w["worst_over_gate"], stats[f"{label}.worst_over_gate"])
    other = kind == "other"
    if other.any():
        stats["other.worst"] = float(err[other].max())
    if record:
        record_error(name, **stats)
        record_error("low_rows.worst_per_template_and_family", **{k: dict(v) for k, v in _WORST.items()})
    assert not bad, (name, len(bad), bad[:8])
    return stats


# ------------------------------------------------------------------------------------------------- every degree, every width
@pytest.mark.parametrize("f,bias,rolled", L.CASES, ids=CASE_IDS)
def test_every_row_within_its_gate(f, bias, rolled):
    """Six families at every degree 0 .. 33, three rows each, stored zeros first / last / in the middle, value == bias, a duplicated
    column, columns 0 and m - 1, rows next to the guards of `indices`, empty rows first, last and between two full pairs, twelve
    bounced rows; the kernels launched are exactly route_low's."""
    case = L.build_case(f, bias, rolled)
    g, names = _run_case(f, bias, rolled)
    _check_names(case, names)
    _gate_rows(f"low_rows[{L.case_id(f, bias, rolled)}]", case, g)


def test_cases_name_every_shipped_instantiation():
    seen = set()
    for c in L.CASES:
        seen |= {n for n in _run_case(*c)[1] if n.startswith(LOW)}
    assert seen == L.every_shipped_name(), sorted(L.every_shipped_name() ^ seen)


def test_launched_kernels_at_every_width():
    """Every f = 1 .. 260, without and with biases, and the rolled layout: rows of 3, 12 and 24 entries and a negative row of 5 (it
    shares the 3-entry row's wave, so both go to the pivoted kernel).  The only test that launches every instantiation."""
    bad = []
    for f, bias, rolled in [(f, b, False) for f in range(1, 261) for b in (0, 1)] + [(129, 1, True)]:
        case = L.launch_case(f, bias, rolled)
        g, names = _solve(case, profile=True)
        _check_names(case, names)
        try:
            _gate_rows(f"low_launch[{L.case_id(f, bias, rolled)}]", case, g, orders=4, record=False)
        except AssertionError as e:
            bad.append(str(e)[:300])
    record_error("low_rows.worst_per_template_and_family", **{k: dict(v) for k, v in _WORST.items()})
    assert not bad, (len(bad), bad[:6])


# ----------------------------------------------------------------------------------------------------------------- pairings
@pytest.mark.parametrize("f,bias,rolled", L.PAIR_WIDTHS, ids=[L.case_id(*c) for c in L.PAIR_WIDTHS])
def test_pairings_and_positions_do_not_change_a_bit(f, bias, rolled):
    """All 81 ordered pairs (dA, dB) in 0 .. 8 and a last row without a partner, then rows of 9 .. 32 entries: the cross blocks of a
    pair's tile are dropped exactly and a longer row has a wave of its own, so every row is bit-identical to the same row solved
    in a CSR of its own, and a second run to the first."""
    case = L.pair_case(f, bias, rolled)
    dev = _Device(case)
    first, names = _solve(case, dev, profile=True)
    _check_names(case, names)
    again = _solve(case, dev)[0]
    assert np.array_equal(first, again), "two runs differ"
    _gate_rows(f"low_pairs[{L.case_id(f, bias, rolled)}]", case, first)
    alone = np.stack([_solve(case.subset(np.array([u])), dev)[0][0] for u in range(case.n)])
    differ = np.flatnonzero((first != alone).any(axis=1))
    assert not differ.size, (len(differ), [(int(u), int(case.degree[u])) for u in differ[:8]])


def test_two_runs_of_a_whole_case_give_the_same_bits():
    for c in ((16, 1, False), (129, 1, True), (200, 0, False)):
        case = L.build_case(*c)
        assert np.array_equal(_run_case(*c)[0], _solve(case)[0]), c


# ------------------------------------------------------------------------------------------------------------------ bounces
@pytest.mark.parametrize("f,bias,rolled,count", L.BOUNCE_WIDTHS, ids=[f"{L.case_id(f, b, r)}-{c}" for f, b, r, c in L.BOUNCE_WIDTHS])
def test_bounced_rows_and_their_partners(f, bias, rolled, count):
    """A negative effective weight -- a negative value, and 0 < value < bias in every bias layout -- in row A and in row B of a pair,
    in a row of 12 and of 24 entries; the partner goes to the pivoted kernel with it.  270 rows on solve_general_kernel's list of
    256 workgroups, 70 on solve_wide_lu_kernel's of 64: the grid-stride loops go round."""
    case = L.bounce_case(f, bias, rolled, count)
    g, names = _solve(case, profile=True)
    _check_names(case, names)
    stats = _gate_rows(f"low_bounce[{L.case_id(f, bias, rolled)}-{count}]", case, g)
    assert "bounced.worst" in stats


@pytest.mark.parametrize("f,bias,k", L.SINGULAR_WIDTHS, ids=[f"f{f}-b{b}-k{k}" for f, b, k in L.SINGULAR_WIDTHS])
def test_exactly_singular_rows_are_counted_and_zero(f, bias, k):
    """v = e_1 with effective weight -1: A = I - e_1 e_1^T in exact arithmetic, pivot column 0 is exactly zero.  fail_count is k,
    those rows of g are exactly 0 (asserted by _gate_rows), every other row -- their pair partners too -- meets its gate."""
    case = L.singular_case(f, bias, k)
    g, names = _solve(case, fails=k, profile=True)
    assert case.route.fallback in names
    assert not g[case.tags == "unit"].any()
    _gate_rows(f"low_singular[f{f}-b{bias}-k{k}]", case, g)
