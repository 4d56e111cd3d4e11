"""tests/low_ref.py -- the reference and the cases tests/test_gpu_low_rows.py is gated on -- checked without a GPU: the d x d forms
against iter_ref.solve_rows_ref (the push-through identity) and against the oracle on a whitened golden half step, route_low against
the names the routing tests pin, the shape of derive_widths(), and, for EVERY case the GPU file builds, the conditions that make
4 E_lr32 + T_x6 a gate a subtly wrong kernel cannot pass: at most 2e-5 on every row, cond(I + E S E) <= 100 on the stiff and the
aligned rows, and neither family emptied by the rule that gets them there."""
import numpy as np
import pytest

import low_ref as L
from conftest import load_golden
from oracle import wmf_oracle as orc

CASE_IDS = [L.case_id(*c) for c in L.CASES]


# --------------------------------------------------------------------------------------------------------------- references
@pytest.mark.parametrize("f,bias,rolled", [(2, 0, False), (4, 1, False), (16, 0, False), (33, 1, False), (64, 0, False), (129, 1, True),
                                            (200, 1, False)])
def test_low_rank_forms_are_the_reference(f, bias, rolled):
    """V_u^T (I + D S)^-1 p = (I + V_u^T D V_u)^-1 V_u^T p: both d x d forms in float64 equal iter_ref.solve_rows_ref to 1e-12 on
    every row of a case, the rows with more entries than features, a stored zero and a negative weight included.  A stiff row of
    fewer entries than features is the exception: cond(I + E S E) <= 100 but the f x f matrix keeps the eigenvalue 1 next to
    w |v|^2 ~ 1e6, so it is the REFERENCE's f x f solve that is good to eps cond(A_u) only -- 1e-10, three orders below any gate;
    there the bound is 8 eps cond_2(A_u)."""
    case = L.build_case(f, bias, rolled)
    ref = case.ref()
    short = (case.degree > 0) & (case.degree <= 33)
    bound = np.maximum(1e-12, 8 * 2.3e-16 * L.R.conditions(case))
    assert (bound[case.family != "stiff"] == 1e-12).all()
    err = L.row_errors(L.ref_lowrank64(case), ref)
    assert (err[short] <= bound[short]).all(), float((err / bound)[short].max())
    assert not L.ref_lowrank64(case)[case.degree == 0].any() and not ref[case.degree == 0].any()
    neg = case.negative()
    assert neg.any() and (case.tags[neg] != "").all()
    for d in (1, 5, 8, 16, 17, 24, 32):
        rows = np.flatnonzero((case.degree == d) & ~neg)
        Vu, w = case.gather(rows)
        assert (w >= 0).all()
        sym = L.symmetric(Vu, w, np.float64)
        assert sym.dtype == np.float64 and (L.row_errors(sym, ref[rows, :f]) <= bound[rows]).all(), (d, L.row_errors(sym, ref[rows, :f]).max())
        assert L.lowrank(Vu, w).dtype == np.float32 and L.symmetric(Vu, w).dtype == np.float32


def test_reference_against_the_oracle_on_a_whitened_golden_case():
    """x_u = L^-T g_u is the oracle's row (tests/test_iter_ref_cpu.py): the d x d form on the rows of at most 32 entries."""
    from test_iter_ref_cpu import _whitened_golden
    g, Yt, bias, G, Lc, V = _whitened_golden()
    f = Yt.shape[1]
    indptr, indices, values = g["C_indptr"].astype(np.int64), g["C_indices"], g["C_data"]
    worst, seen = 0.0, 0
    for u in range(len(indptr) - 1):
        idx = indices[indptr[u]: indptr[u + 1]]
        if not 0 < len(idx) <= 32:
            continue
        w32 = values[indptr[u]: indptr[u + 1]].astype(np.float32) - bias[idx].astype(np.float32)
        got = L.lowrank(V[idx][None], w32[None], np.float64)[0]
        want = orc.solve_row(G, Yt, idx, w32.astype(np.float64))
        x = np.linalg.solve(Lc.T, got)
        worst = max(worst, np.linalg.norm(x - want) / np.linalg.norm(want))
        seen += 1
    assert seen >= 10 and worst <= 1e-5, (seen, worst)


def test_split8_is_the_kernels_split():
    """hi + lo is 256 v to 2^-22 while lo is a normal f16 number; the tile differs from S by the dropped lo lo products only."""
    rng = np.random.default_rng(0)
    v = (rng.standard_normal(4096) * 0.1).astype(np.float32)
    hi, lo = L.split8(v)
    assert hi.dtype == lo.dtype == np.float16
    s = 256.0 * v.astype(np.float64)
    assert (np.abs(hi.astype(np.float64) + lo.astype(np.float64) - s) <= 2.0 ** -21 * np.abs(s) + 2.0 ** -25).all()
    Vu = (rng.standard_normal((3, 12, 64)) * 0.05).astype(np.float32)
    S = Vu.astype(np.float64) @ Vu.astype(np.float64).transpose(0, 2, 1)
    assert np.abs(L.x6_tile(Vu, 64) - S).max() <= 64 * 2.0 ** -20 * 0.05 ** 2 * 16
    assert np.array_equal(L.x6_tile(Vu[:, :, :1], 0), S * 0 + Vu[:, :, :1].astype(np.float64) @ Vu[:, :, :1].astype(np.float64).transpose(0, 2, 1))
    tiny = np.float32(1e-6)                                          # 256 v = 2.6e-4: the low part is a subnormal f16 number
    hi, lo = L.split8(tiny)
    assert 0 < abs(float(lo)) < 6.2e-5 and abs(float(hi) + float(lo) - 256e-6) <= 3e-8


# ------------------------------------------------------------------------------------------------------------- the dispatch
def test_route_low_at_the_widths_the_routing_tests_pin():
    """tests/test_gpu_routing.py's ROUTES, read off the library: the short-row kernels and the pivoted fallback are route_low's."""
    import test_gpu_routing as T
    kinds = ("solve_pair_kernel", "solve_low_kernel", "solve_general_kernel", "solve_wide_lu_kernel")
    assert len(T.CASES) == 14
    for k, bias, rolled in T.CASES:
        names = {n for n in T.ROUTES[T.case_id(k, bias, rolled)] if n.startswith(kinds)}
        r = L.route_low(k + bias, bias, bool(rolled))
        assert names == L.low_names(r) | {r.fallback}, (k, bias, rolled, sorted(names))
    assert L.route_low(129, 1, True).bstride == 3 and L.route_low(129, 1, False).bstride == 2 and L.route_low(129, 0, True).bstride == 1
    assert L.route_low(144, 0).fallback == "solve_general_kernel<9>" and L.route_low(145, 0).fallback == "solve_wide_lu_kernel"


def test_shape_of_the_derived_widths():
    W = L.WIDTHS
    assert 65 <= len(W) <= 75 and {1, 2, 3, 4, 260} <= set(W) and 140 <= len(L.CASES) <= 200
    routes = [L.route_low(f, b) for f in W for b in (0, 1)]
    for nch in range(1, 18):
        assert {r.last1 for r in routes if r.nch == nch} == {False, True}, nch
    assert {r.nch % 2 for r in routes if r.x6} == {0, 1}             # whole chunks; whole chunks and one more piece
    assert {f for f in W if L.route_low(f, 1).split} == {17, 33, 65, 81, 97, 129}
    for f in range(2, 261):                                          # an edge and its left neighbour are both cases
        if L._key(f) != L._key(f - 1):
            assert f in W and f - 1 in W
    named = {n for f, b, r in L.CASES for n in L.low_names(L.route_low(f, b, r))}
    assert named == L.every_shipped_name() and len(named) >= 80, sorted(L.every_shipped_name() - named)
    assert {L.route_low(f, b, r).bstride for f, b, r in L.CASES} == {1, 2, 3}


# -------------------------------------------------------------------------------------------------------------------- cases
def _check_structure(case, name):
    """The special rows are there, where the kernels meet them."""
    f, bias = case.f, case.bias
    deg, tags, fam = case.degree, case.tags, case.family
    assert case.n <= 1500 and case.V.shape[0] == 600
    assert deg[0] == 0 and deg[-1] == 0 and deg[1] > 0 and deg[-2] > 0     # an empty row first and last; entries next to both guards
    assert tags[1] == tags[-2] == "straddle" and fam[1] == fam[-2] == "near"
    pairs = case.pairs()
    full = [i for i, (a, b) in enumerate(pairs) if b >= 0 and deg[a] == 8 and deg[b] == 8 and tags[a] == "full"]
    between = [i for i in full if i + 2 in full and deg[pairs[i + 1][0]] == 0]
    assert between, name                                             # (8, 8), (0, 8), (8, 8)
    neg = case.negative()
    for a, b in pairs[1:4]:                                          # negative rows of 5 entries and their partners
        assert neg[a] and not neg[b] and tags[b] == "partner", name
    assert {int(d) for d in deg[neg]} == {5, 12, 24}
    bounced = case.bounced()
    assert bounced.sum() == 12 and set(fam[bounced]) == {"negative"}
    U, w = case.inputs()
    at = {t: np.flatnonzero(tags == t) for t in L.STRUCTURE_TAGS}
    assert all((fam[at[t]] == "structure").all() for t in at)
    for t in ("zero_first", "zero_mid", "zero_last", "eqbias", "dup", "ends"):
        assert {int(d) for d in deg[at[t]]} == {6, 12, 24}, (name, t)
    for t, pos in (("zero_first", 0), ("zero_last", -1)):
        for u in at[t]:
            lo, hi = case.indptr[u], case.indptr[u + 1]
            assert w[lo:hi][pos] == 0 and case.values[lo:hi][pos] == 0 and (np.delete(w[lo:hi], pos) > 0).all()
    for u in at["zero_mid"]:
        lo, hi = case.indptr[u], case.indptr[u + 1]
        assert w[lo + (hi - lo) // 2] == 0 and case.values[lo + (hi - lo) // 2] == 0
    for u in at["eqbias"]:
        lo, hi = case.indptr[u], case.indptr[u + 1]
        mid = lo + (hi - lo) // 2
        assert w[mid] == 0 and (case.values[mid] == 0.125) == bool(bias)   # value == bias != 0 wherever there is a bias
    for u in at["dup"]:
        idx = case.indices[case.indptr[u]: case.indptr[u + 1]]
        assert len(set(idx.tolist())) == len(idx) - 1
    for u in at["ends"]:
        idx = case.indices[case.indptr[u]: case.indptr[u + 1]]
        assert idx[0] == 0 and idx[-1] == 599
    # every family at every degree, REPS rows each, none dropped; above f entries the first two families only
    plain = tags == ""
    for d in range(1, 34):
        for fm in L.FAMILIES:
            got = int((plain & (deg == d) & (fam == fm)).sum())
            assert got == (L.REPS if fm in L.families_at(f, d) else 0), (name, d, fm, got)
    assert int((deg == 0).sum()) >= 4
    assert (w[np.repeat(~neg, deg)] >= 0).all()


@pytest.mark.parametrize("f,bias,rolled", L.CASES, ids=CASE_IDS)
def test_cases_keep_their_conditions(f, bias, rolled):
    """(The float64 reference here is the d x d form, test_low_rank_forms_are_the_reference: 1e-12 from solve_rows_ref.)"""
    name = L.case_id(f, bias, rolled)
    case = L.build_case(f, bias, rolled)
    _check_structure(case, name)
    gate, kind, E, ys = L.gates(case, L.ref_lowrank64(case))
    solved = np.isin(kind, L.CLASSES)
    assert solved.sum() >= 200 and (kind[(case.degree > 0) & (case.degree <= 32) & ~case.bounced()] != "other").all()
    assert (gate[solved] > 0).all() and gate[solved].max() <= L.GATE_CAP, (name, float(gate[solved].max()), int(np.argmax(np.where(solved, gate, 0))))
    assert (kind[case.degree == 33] == "other").all() and (kind[case.degree == 0] == "empty").all()
    if not case.route.x6:
        assert not ys["t_x6"].any()
    else:
        assert (ys["t_x6"][solved] > 0).mean() > 0.9 and ys["t_x6"].max() <= 5e-6
    tamed = solved & np.isin(case.family, L.TAMED)
    assert ys["cond"][tamed].max() <= L.COND_MAX, (name, float(ys["cond"][tamed].max()))
    assert E["bounced"] <= 2e-6, (name, E["bounced"])                # the negative rows are near-identity rows: LAPACK's float32 is fine
    if f >= 64:                                                      # the rule does not empty the stiff family
        U, w = case.inputs()
        wmax = np.maximum.reduceat(w, case.indptr[:-1][case.degree > 0])
        top = np.zeros(case.n)
        top[case.degree > 0] = wmax
        for c in range(3):
            sel = solved & (case.family == "stiff") & (case.cls == c)
            assert (top[sel] >= 1e5).any(), (name, L.CLASSES[c], float(top[sel].max()))
        for c in range(3):                                           # ... nor the aligned one: weights of 1e2 and more
            sel = solved & (case.family == "aligned") & (case.cls == c)
            assert (top[sel] >= 1e2).any(), (name, L.CLASSES[c], float(top[sel].max()))


# ------------------------------------------------------------------------------------------------------- the widened margins
EMULATED_WIDTHS = (1, 2, 4, 16, 33, 64, 129, 144, 145, 200, 258)


def _emulated_ratios(case):
    """{(family, class) or "bounced": worst restated error / yardstick}."""
    ref = L.ref_lowrank64(case)
    gate, kind, E, ys = L.gates(case, ref)
    out = {}
    for key, e in E.items():
        if key == "bounced":
            rows = np.flatnonzero(kind == "bounced")
            out[key] = L.emulated_errors(case, ref, rows, pivoted=True).max() / e
        else:
            rows = np.flatnonzero((kind == key[1]) & (case.family == key[0]))
            out[key] = L.emulated_errors(case, ref, rows).max() / e
    return out


def test_restated_kernel_arithmetic_is_the_reference():
    case = L.build_case(33, 1, False)
    ref = case.ref()
    for d in (1, 8, 9, 16, 17, 20, 32):
        rows = np.flatnonzero((case.degree == d) & ~case.negative())
        assert L.emulated_errors(case, ref, rows).max() <= 2e-5
    rows = np.flatnonzero(case.bounced())
    assert L.emulated_errors(case, ref, rows, pivoted=True).max() <= 2e-6


@pytest.mark.parametrize("f", EMULATED_WIDTHS)
def test_margins_against_the_restated_kernel_arithmetic(f):
    """Every (family, class) at MARGIN has a restated figure below MARGIN; the two widened kinds have theirs below the figure their
    margin is 1.5 times of (and the figure is reached: the aligned rows' at f = 125, the bounced rows' at f = 258)."""
    for bias in (0, 1):
        case = L.build_case(f, bias)
        for key, ratio in _emulated_ratios(case).items():
            if key == "bounced":
                assert ratio <= L.EMULATED_BOUNCED, (f, bias, key, ratio)
            elif L.margin_of(case, *key) == L.MARGIN:
                assert ratio <= L.MARGIN, (f, bias, key, ratio)
            else:
                assert ratio <= L.EMULATED_ALIGNED32, (f, bias, key, ratio)
    if f == 258:
        assert _emulated_ratios(L.build_case(258, 0))["bounced"] >= 0.9 * L.EMULATED_BOUNCED


def test_aligned_rows_in_the_block_form_at_every_case():
    worst = 0.0
    for c in L.CASES:
        case = L.build_case(*c)
        ref = L.ref_lowrank64(case)
        ys = L.yardsticks(case, ref)
        rows = np.flatnonzero((case.family == "aligned") & (case.cls == 2))
        if len(rows):
            worst = max(worst, L.emulated_errors(case, ref, rows).max() / ys["e_lr"][rows].max())
    assert 0.8 * L.EMULATED_ALIGNED32 <= worst <= L.EMULATED_ALIGNED32, worst
    assert L.MARGIN_ALIGNED32 == 1.5 * L.EMULATED_ALIGNED32 and L.MARGIN_BOUNCED == 1.5 * L.EMULATED_BOUNCED


def test_the_other_cases_are_what_their_tests_need():
    for f, bias, rolled in L.PAIR_WIDTHS:
        case = L.pair_case(f, bias, rolled)
        pairs = case.pairs()
        assert len(pairs) == 82 and pairs[-1][1] == -1 and not case.negative().any()
        assert {(int(case.degree[a]), int(case.degree[b])) for a, b in pairs[:-1]} == {(a, b) for a in range(9) for b in range(9)}
        assert sorted(case.degree[163:].tolist()) == list(range(9, 33)) and case.n % 2 == 1
        r = L.route_low(f, bias, rolled)
        assert (r.x6, r.split, r.bstride) == {50: (False, False, 1), 64: (True, False, 1), 81: (False, True, 2), 129: (True, True, 3)}[f]
    for f, bias, rolled, count in L.BOUNCE_WIDTHS:
        case = L.bounce_case(f, bias, rolled, count)
        neg, b = case.negative(), case.bounced()
        assert b.sum() >= count and case.n <= 1500 and (b & ~neg).any()
        assert {int(d) for d in case.degree[neg]} == {5, 6, 12, 24}
        pairs = case.pairs()
        assert any(neg[a] and not neg[p] for a, p in pairs if p >= 0) and any(neg[p] and not neg[a] for a, p in pairs if p >= 0)
        assert set(case.tags[neg]) == ({"neg", "negbias"} if bias else {"neg"})
        assert (~b & (case.degree > 0)).sum() >= 10
    assert max(c for f, b, r, c in L.BOUNCE_WIDTHS if f <= 144) > 256 and max(c for f, b, r, c in L.BOUNCE_WIDTHS if f > 144) > 64
    for f, bias, k in L.SINGULAR_WIDTHS:
        case = L.singular_case(f, bias, k)
        unit = np.flatnonzero(case.tags == "unit")
        assert len(unit) == k
        U, w = case.inputs()
        for u in unit:
            e = case.indptr[u]
            assert case.degree[u] == 1 and w[e] == -1 and U[case.indices[e], 0] == 1 and not U[case.indices[e], 1:].any()
        assert not case.ref()[unit].any() and np.isfinite(case.ref()).all()
    assert {f for f, b, k in L.SINGULAR_WIDTHS} == {16, 129, 200}
    for f, bias, rolled in ((1, 0, False), (129, 1, True), (260, 1, False)):
        case = L.launch_case(f, bias, rolled)
        assert case.degree.tolist() == [3, 12, 24, 5] and case.bounced().tolist() == [True, False, False, True]   # (the two short rows share a wave)
