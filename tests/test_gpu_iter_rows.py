"""The float32 matrix-free iteration (csrc/wmf_iter.hip) PER ROW through wmf_plan_create / wmf_solve_rows_ex / wmf_plan_iter_stats,
against tests/iter_ref.py: every shipped instantiation, every degree, every path, and the steady state of its row pipeline.

The whitened side is an argument of wmf_solve_rows, so a case needs no half step: a hand-made V of 600 rows with norms 0.03 and
weights scaled per row put any tau_plus, tau_minus and spectrum into a row of any length (iter_ref.FAMILIES).  Every input sits
between guard rows of NaN (an index guard points into them), the output between sentinel rows.

Gates (a row's error is ||got - ref|| / ||ref|| against the float64 reference of exactly the uploaded float32 arrays):
    a row the iteration solved   4 E32 + 1.2e-7 chi / alpha -- E32 the worst row error of NumPy's float32 solve over the same case
                                 and family (measured here against the same reference, never taken from the device), the second
                                 term the truncation the stopping test admits.  Margin 4: the kernel's sums of up to 256 entries
                                 run in lane / wave order, BLAS's in its own; emulating the kernel's arithmetic in NumPy float32
                                 gave 1.1 - 1.6e-7 where E32 was 1.1 - 1.4e-7.
    any other row                tests/test_gpu_parity.py's row tolerance of its width (5e-4, 1e-3 above f = 144): the elimination
                                 kernels' (split-f16 operands).
Paths: wmf_plan_iter_stats must give EXACTLY the rows done / bounced / on the Chebyshev recurrence that iter_ref.policy predicts in
float64 (tests/test_iter_ref_cpu.py asserts the margins that make the prediction exact), the applications within +- done.
Measured on an MI355X (profiles/r14_iter_rows.json): a solved row is 0.2 .. 1.43 x E32 of its family, at most 0.27 of its gate, worst
4.5e-7 (Chebyshev on the aligned rows, E32 4.5e-7); the other rows 5.2e-7 (f <= 144) and 2.8e-6, under WMF_DBG_NO_ITER 7.7e-7 and 7.8e-6."""
import numpy as np
import pytest
import torch

import iter_ref as R
from conftest import record_error

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
GUARD = 4
HALF_ROW, WIDE_ROW = 5e-4, 1e-3                                      # tests/test_gpu_parity.py
NO_ITER = 268435456
SOLVE_ROLLED = 1

MAIN_IDS = [R.case_id(*c) for c in R.MAIN]
MINOR = R.minor_cases()
ALL_CASES = [("main", *c) for c in R.MAIN] + [("minor", f, b, False) for f, b in MINOR]
ALL_IDS = [f"{kind}-{R.case_id(f, b, r)}" for kind, f, b, r in ALL_CASES]


def _case(kind, f, bias, rolled):
    return R.build_case(f, bias, rolled) if kind == "main" else R.minor_case(f, bias)


# ------------------------------------------------------------------------------------------------------------------ helpers
def _guarded(a, fill, dtype):
    """a device copy of `a` between GUARD rows (elements, for a vector) of `fill`; returns (buffer, view of the payload)."""
    a = np.array(a, dtype=dtype, order="C")                         # (a copy: the cases' arrays are read-only)
    buf = torch.full((a.shape[0] + 2 * GUARD, *a.shape[1:]), fill, dtype=torch.from_numpy(a).dtype, device="cuda")
    buf[GUARD: GUARD + a.shape[0]] = torch.from_numpy(a).cuda()
    return buf, buf[GUARD: GUARD + a.shape[0]]


class _Device:
    """The fixed side of a case on the device: V and the pairs / bias vector between NaN rows."""

    def __init__(self, case):
        self.V = _guarded(case.V, float("nan"), np.float32)
        side = case.side if case.side is not None else case.bias_fixed
        self.side = _guarded(side, float("nan"), np.float32) if side is not None else (None, None)


def _upload_rows(case):
    """indptr as it is (a guard of it could only be read as an offset), indices between guards that point into V's NaN rows,
    values between NaNs."""
    m = case.V.shape[0]
    ix = _guarded(case.indices, 0, np.int32)
    ix[0][:GUARD] = -1
    ix[0][GUARD + len(case.indices):] = m
    return torch.from_numpy(case.indptr.copy()).cuda(), ix, _guarded(case.values, float("nan"), np.float32)


def _launches(lib, run):
    from recmodel_amd import _lib
    torch.cuda.synchronize()
    lib.wmf_profile_reset()
    lib.wmf_profile_enable(1)
    try:
        out = run()
        torch.cuda.synchronize()
    finally:
        lib.wmf_profile_enable(0)
    names = {name.replace(" [bounced]", "") for name, *_ in _lib.profile_table(lib)}
    lib.wmf_profile_reset()
    return out, names


def _solve(case, dev=None, debug=0, profile=False):
    """One wmf_solve_rows_ex over the case in a plan of its own.  Returns (g [n, ld], iter stats (4), plan stats (14), kernel names)."""
    from recmodel_amd import _lib
    from recmodel_amd.engine import HipKernels
    K = HipKernels()
    lib = K.lib
    dev = dev or _Device(case)
    ipd, (ixbuf, ix), (vbuf, vals) = _upload_rows(case)
    n, f, ld = case.n, case.f, case.ld
    gbuf = torch.full((n + 2 * GUARD, ld), SENTINEL, dtype=torch.float32, device="cuda")
    fail = torch.zeros(4, dtype=torch.int32, device="cuda")
    fail[1:] = 77
    plan, pstats = K.plan_create(np.ascontiguousarray(case.indptr), n, f, case.bias)
    try:
        assert lib.wmf_debug_set_flags(debug) == 0
        K.plan_iter_stats(plan)

        def run():
            K.solve_rows(plan, dev.V[1], dev.side[1], ipd, ix, vals, n, f, ld, gbuf[GUARD:], fail, flags=SOLVE_ROLLED if case.rolled else 0)
        names = _launches(lib, run)[1] if profile else run()
        istats = K.plan_iter_stats(plan)                             # (synchronises)
    finally:
        lib.wmf_debug_set_flags(0)
        K.plan_destroy(plan)
    got = gbuf.cpu().numpy()
    assert np.all(got[:GUARD] == SENTINEL) and np.all(got[GUARD + n:] == SENTINEL), "a write outside the output rows"
    assert fail.tolist() == [0, 77, 77, 77], fail.tolist()
    g = got[GUARD: GUARD + n]
    assert not (g == SENTINEL).any(), ("a sentinel survived", np.flatnonzero((g == SENTINEL).any(axis=1))[:8])
    assert np.isfinite(g).all(), ("a guard row was read", np.flatnonzero(~np.isfinite(g).all(axis=1))[:8])
    assert not g[:, f:].any(), "padding columns of g are not exactly 0"
    return g, tuple(int(x) for x in istats), pstats, names


_REF, _RUNS = {}, {}


def _reference(key, case):
    """float64 rows, NumPy float32 rows' errors and policy()'s prediction of a case, computed once."""
    if key not in _REF:
        ref = case.ref()
        for a in (ref,):
            a.setflags(write=False)
        _REF[key] = {"ref": ref, "e32": R.row_errors(case.f32(), ref), "final": case.predict()[0]}
    return _REF[key]


def _run_case(kind, f, bias, rolled):
    key = (kind, f, bias, rolled)
    if key not in _RUNS:
        _RUNS[key] = _solve(_case(*key), profile=True)
    return _RUNS[key]


def _gate_rows(name, case, g, refs, iteration_on=True):
    """Per-row gates; returns the figures to record."""
    ref, e32, final = refs["ref"], refs["e32"], refs["final"]
    err = R.row_errors(g, ref)
    assert not g[case.degree == 0].any(), (name, "a row without entries is not exactly 0")
    solved = np.array([iteration_on and p is not None and p["path"] in R.SOLVED for p in final])
    loose = WIDE_ROW if case.f > 144 else HALF_ROW
    stats, bad = {}, []
    for fam in sorted(set(case.family[solved])):
        sel = solved & (case.family == fam)
        E32 = float(e32[sel].max())
        gate = np.array([4 * E32 + R.EPS * final[u]["chi"] / final[u]["alo"] for u in np.flatnonzero(sel)])
        stats[f"{fam}.worst"], stats[f"{fam}.E32"] = float(err[sel].max()), E32
        stats[f"{fam}.ratio_to_E32"] = float(err[sel].max() / E32)
        stats[f"{fam}.worst_over_gate"] = float((err[sel] / gate).max())
        bad += [(int(u), fam, int(case.degree[u]), float(err[u]), float(gt)) for u, gt in zip(np.flatnonzero(sel), gate) if not err[u] <= gt]
    rest = ~solved & (case.degree > 0)
    if rest.any():
        stats["eliminated.worst"] = float(err[rest].max())
        bad += [(int(u), "eliminated", int(case.degree[u]), float(err[u]), loose) for u in np.flatnonzero(rest) if not err[u] <= loose]
    record_error(name, **stats)
    print(name, {k: f"{v:.3e}" for k, v in stats.items()})
    assert not bad, (name, bad[:8])
    return stats


# ------------------------------------------------------------------------------------------------------------------ routing
def test_plan_candidates_at_every_width():
    """wmf_plan_stats()[12 / 13] -- rows and entries the plan hands to the iteration -- on degrees {32, 33, dmax, dmax + 1} at
    every (f, bias), f = 1 .. 260: what iter_ref.iter_dmax says (at a width without a kernel: none of 32, 33, 144, 256)."""
    from recmodel_amd.engine import HipKernels
    K = HipKernels()
    for f in range(1, 261):
        for bias in (0, 1):
            dmax = R.iter_dmax(f, bias)
            deg = np.array([32, 33, dmax, dmax + 1] if dmax else [32, 33, 144, 256])
            indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
            plan, stats = K.plan_create(indptr, len(deg), f, bias)
            K.plan_destroy(plan)
            cand = deg[(deg >= 33) & (deg <= dmax)]
            assert (int(stats[12]), int(stats[13])) == (len(cand), int(cand.sum())), (f, bias, stats[12:14], dmax)


@pytest.mark.parametrize("kind,f,bias,rolled", ALL_CASES, ids=ALL_IDS)
def test_profile_names_exactly_the_routed_kernels(kind, f, bias, rolled):
    case = _case(kind, f, bias, rolled)
    _, _, pstats, names = _run_case(kind, f, bias, rolled)
    assert int(pstats[12]) == int(case.candidate.sum()) and int(pstats[13]) == int(case.degree[case.candidate].sum())
    assert {n for n in names if n.startswith("solve_iter_kernel")} == set(R.route(f, bias, rolled)), sorted(names)


def test_main_cases_reach_every_shipped_instantiation():
    seen = set()
    for c in R.MAIN:
        seen |= {n for n in _run_case("main", *c)[3] if n.startswith("solve_iter_kernel")}
    every = {n for f in range(1, 261) for b in (0, 1) for r in (False, True) for n in R.route(f, b, r)}
    assert seen == every, sorted(every ^ seen)


# ------------------------------------------------------------------------------------------------- every degree, every path
@pytest.mark.parametrize("kind,f,bias,rolled", ALL_CASES, ids=ALL_IDS)
def test_every_row_within_its_gate(kind, f, bias, rolled):
    """Main widths: families A and D at every d = 31 .. dmax + 2, the others at the slot and register edges; the other widths:
    A, C, D at the edges.  A stored zero, a duplicated column, empty rows; rows 0 and m - 1 of the fixed side are gathered."""
    case = _case(kind, f, bias, rolled)
    g = _run_case(kind, f, bias, rolled)[0]
    _gate_rows(f"iter_rows[{kind}-{R.case_id(f, bias, rolled)}]", case, g, _reference((kind, f, bias, rolled), case))


@pytest.mark.parametrize("kind,f,bias,rolled", ALL_CASES, ids=ALL_IDS)
def test_paths_are_exactly_the_predicted_ones(kind, f, bias, rolled):
    """done, bounced and cheb of wmf_plan_iter_stats equal policy()'s counts -- at ldv = 128 a row counted under cheb went through
    stage 1's hand-over and was solved by stage 2 --, the applications agree within one per solved row."""
    case = _case(kind, f, bias, rolled)
    done, bounced, apps, cheb = _run_case(kind, f, bias, rolled)[1]
    want = case.expected_stats(_reference((kind, f, bias, rolled), case)["final"])
    assert (done, bounced, cheb) == (want[0], want[1], want[3]), ((done, bounced, apps, cheb), want)
    assert abs(apps - want[2]) <= want[0], ((done, bounced, apps, cheb), want)
    if not case.dmax:
        assert (done, bounced, apps, cheb) == (0, 0, 0, 0)


# ------------------------------------------------------------------------------------------------------------- the pipeline
@pytest.mark.parametrize("f,bias,rolled", R.MAIN, ids=MAIN_IDS)
def test_pipeline_in_its_steady_state(f, bias, rolled):
    """4 cap + 37 rows, clones of 32 distinct ones in random order: every workgroup of the launch (stage 2 at ldv = 128: 512 over
    the whole list) solves four or five rows of different lengths, prefetching two or three rows ahead.  A row's path and bits
    depend on its own data only (csrc/wmf_iter.hip): every clone is bit-identical to the row solved alone in a one-row plan and
    to its second run; the 32 distinct rows meet the gates."""
    distinct, clones, which = R.pipeline_case(f, bias, rolled)
    dev = _Device(distinct)
    first, stats, _, names = _solve(clones, dev, profile=True)
    again = _solve(clones, dev)[0]
    assert np.array_equal(first, again), "two runs differ"
    assert {n for n in names if n.startswith("solve_iter_kernel")} == set(R.route(f, bias, rolled))
    refs = _reference(("pipeline", f, bias, rolled), distinct)
    alone = np.stack([_solve(R.single_row(distinct, k), dev)[0][0] for k in range(32)])
    _gate_rows(f"iter_pipeline[{R.case_id(f, bias, rolled)}]", distinct, alone, refs)
    differ = np.flatnonzero((first != alone[which]).any(axis=1))
    assert not differ.size, (len(differ), [(int(u), int(which[u]), int(clones.degree[u])) for u in differ[:8]])
    count = np.bincount(which, minlength=32)
    final = refs["final"]
    done = sum(int(c) for c, p in zip(count, final) if p["path"] in R.SOLVED)
    cheb = sum(int(c) for c, p in zip(count, final) if p["path"] in ("switch", "chebyshev"))
    apps = sum(int(c) * p["applications"] for c, p in zip(count, final) if p["path"] in R.SOLVED)
    assert (stats[0], stats[1], stats[3]) == (done, clones.n - done, cheb) and done == clones.n, (stats, done, cheb)
    assert abs(stats[2] - apps) <= done, (stats, apps)


# --------------------------------------------------------------------------------------------------------------- the switch
@pytest.mark.parametrize("f,bias,rolled", R.MAIN, ids=MAIN_IDS)
def test_iteration_switched_off(f, bias, rolled):
    """WMF_DBG_NO_ITER: no iteration kernel runs, the counters stay zero, and every row -- those the iteration would have solved
    too -- is within the elimination kernels' stated tolerance."""
    case = R.build_case(f, bias, rolled)
    refs = _reference(("main", f, bias, rolled), case)
    g, stats, _, names = _solve(case, debug=NO_ITER, profile=True)
    assert stats == (0, 0, 0, 0), stats
    assert not any(n.startswith("solve_iter_kernel") for n in names), sorted(names)
    _gate_rows(f"iter_rows_no_iter[{R.case_id(f, bias, rolled)}]", case, g, refs, iteration_on=False)
    on = _run_case("main", f, bias, rolled)[0]
    solved = np.array([p is not None and p["path"] in R.SOLVED for p in refs["final"]])
    assert (on[solved] != g[solved]).any(axis=1).mean() >= 0.9, "the iteration's rows are the elimination kernels' bits"
