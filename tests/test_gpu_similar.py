"""wmf_row_inv_norms and wmf_similar_topn through the C ABI, per element (csrc/wmf_similar.hip): the neighbours of rows of a factor
matrix, by dot product or cosine over the feature columns, by the catalogue scan of wmf_recommend_topn with a second scoring rule.

The vocabulary of tests/test_gpu_recommend.py: the same widths, bias settings and leading dimensions, the same two input classes
(tests/serving_ref.py) -- EXACT, integers with a few all-zero rows, where the device must equal tests/similar_ref.py bit for bit (the
dots are exact, the two float32 multiplications are repeated in NumPy) and equal scores are real ties, and ROUNDED, standard normal,
held to the derived bound B_cos(q, j).  A catalogue of 300 rows and 40 queries that are rows of it."""
import functools

import numpy as np
import pytest
import torch

import recommend_ref as rref
import serving_ref as ref
import similar_ref as sref
from conftest import record_error
from scan_cases import N_PATTERNS, _api, _check_rounded_order, _constant, _dev, _ld, _seen_rows, case

pytestmark = pytest.mark.gpu

N_QUERIES, N_ROWS = 40, 300
GRID_QUERIES, GRID_ROWS, GRID_TOPN, GRID_SLICES = (1, 15, 16, 17, 33, 40), (1, 15, 16, 17, 255, 256, 257, 300), (1, 2, 10, 64, 128), (0, 1, 2, 3, 7, 64)
GRID_CASES = ((129, 1), (64, 0))
SENTINEL = -12345.0
# row 0, the last row, the rows around a wave's 16, row 2 twice (batch positions 2 and 9); the rest spread over the catalogue
QUERIES = np.array([0, N_ROWS - 1, 2, 15, 16, 17, 31, 32, 33, 2] + [(37 * b + 5) % N_ROWS for b in range(10, N_QUERIES)])
assert len(QUERIES) == N_QUERIES and len(np.unique(QUERIES)) == N_QUERIES - 1


# ------------------------------------------------------------------------------------------------------------------ helpers
@functools.lru_cache(maxsize=None)
def _catalogue(f, cls):
    """The catalogue of a width; in the EXACT class the queries include all-zero rows (inverse norm 0: every cosine ties at 0)."""
    make = ref.exact_factors if cls == "exact" else ref.rounded_factors
    C = make(N_ROWS, f, 10 * f + 2)
    if cls == "exact":
        C[[QUERIES[3], QUERIES[12]]] = 0
    C.setflags(write=False)
    return C


@functools.lru_cache(maxsize=None)
def _exact_dots(f, bias):
    """int64 [N_QUERIES, N_ROWS] feature dots of the EXACT class.  Computed once, never written."""
    C = _catalogue(f, "exact")
    D = sref.dot_matrix_int(C, C, QUERIES, np.arange(N_ROWS), bias)
    D.setflags(write=False)
    return D


@functools.lru_cache(maxsize=None)
def _rounded_cosines(f, bias):
    """(float64 cosines [N_QUERIES, N_ROWS], B_cos) of the ROUNDED class.  Computed once, never written."""
    C = _catalogue(f, "rounded")
    rows = np.arange(N_ROWS)
    inv = sref.inv_norms_f64(C, bias)
    cos = sref.cosine_f64(sref.dot_matrix_f64(C, C, QUERIES, rows, bias), inv[QUERIES], inv)
    bound = sref.cos_bound(sref.dot_bound(C, C, QUERIES, rows, bias), inv[QUERIES], inv, cos)
    cos.setflags(write=False)
    bound.setflags(write=False)
    return cos, bound


def _scale_settings(C, bias):
    """{name: (scales of the query rows by ROW ID, scales of the catalogue rows)}: none, the reference inverse norms, and powers of
    two under which different integer dots tie."""
    inv = sref.inv_norms_ref(C, bias)
    i = np.arange(len(C))
    return {"none": None, "norms": (inv, inv), "powers": ((2.0 ** (i % 2)).astype(np.float32), (2.0 ** -(i % 3)).astype(np.float32))}


def _scaled(D, scales, query_rows):
    if scales is None:
        return D.astype(np.float32)
    return sref.scale_f32(D, scales[0][query_rows], scales[1])


class _Similar:
    """wmf_similar_topn on prefixes of one query list and of one catalogue.  The outputs are one row longer than asked for: the
    spare row keeps its sentinel."""

    def __init__(self, Qf, Cf, f, ld, bias, query_idx, scales=None):
        self.Qd = _dev(ref.padded(Qf, ld))
        self.Cd = self.Qd if Cf is Qf else _dev(ref.padded(Cf, ld))
        self.args = (f, ld, bias)
        self.query_idx = _dev(query_idx, np.int32)
        self.scales = None if scales is None else (_dev(scales[0], np.float32), _dev(scales[1], np.float32))

    def __call__(self, n_queries, n_rows, topn, n_slices, exclude_self, excl=None, scores=True, count=True):
        _lib, lib, _ptr, _stream = _api()
        f, ld, bias = self.args
        ws = torch.empty(int(lib.wmf_similar_workspace_bytes(n_queries, topn, n_slices)), dtype=torch.uint8, device="cuda")
        rows = torch.full((n_queries + 1, topn), -7, dtype=torch.int32, device="cuda")
        sc = torch.full((n_queries + 1, topn), SENTINEL, dtype=torch.float32, device="cuda")
        cnt = torch.full((n_queries + 1,), -7, dtype=torch.int32, device="cuda")
        ip_d = idx_d = None
        if excl is not None:
            indptr, indices = rref.csr_of(excl)
            assert len(indptr) == n_queries + 1
            ip_d, idx_d = _dev(indptr, np.int64), _dev(indices, np.int32)
        sq, si = self.scales if self.scales is not None else (None, None)
        _lib.check(lib.wmf_similar_topn(_ptr(self.Qd), _ptr(self.Cd), f, ld, bias, _ptr(sq), _ptr(si), _ptr(self.query_idx), n_queries, n_rows,
                                        int(exclude_self), _ptr(ip_d), _ptr(idx_d), topn, n_slices, _ptr(rows), _ptr(sc) if scores else None,
                                        _ptr(cnt) if count else None, _ptr(ws), ws.numel(), _stream()))
        rows, sc, cnt = rows.cpu().numpy(), sc.cpu().numpy(), cnt.cpu().numpy()
        assert (rows[-1] == -7).all() and (sc[-1] == SENTINEL).all() and cnt[-1] == -7, "written past the outputs"
        if not scores:
            assert (sc == SENTINEL).all()
        if not count:
            assert (cnt == -7).all()
        return rows[:-1], (sc[:-1] if scores else None), (cnt[:-1] if count else None)


def _same_bits(a, b):
    return all((x is None and y is None) or np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))


def _check_exact(got, S, query_rows, exclude_self, excl, n_rows, topn, what):
    """Rows, scores and counts bit for bit those of similar_ref on the float32 scores S [batch, catalogue]."""
    rows, sc, cnt = got
    want = [sref.similar_ref(S[b, :n_rows], q if exclude_self else None, [] if excl is None else excl[b], topn) for b, q in enumerate(query_rows)]
    want_rows = rref.padded_rows(want, topn, -1, np.int32)
    assert np.array_equal(rows, want_rows), (what, np.argwhere(rows != want_rows)[:5])
    if cnt is not None:
        assert np.array_equal(cnt, [len(w) for w in want]), what
    if sc is not None:
        valid = want_rows >= 0
        want_sc = S[np.repeat(np.arange(len(query_rows)), valid.sum(axis=1)), want_rows[valid]] + np.float32(0.0)      # (-0.0 = +0.0)
        assert (sc[~valid] == -np.inf).all() and np.array_equal(sc[valid].view(np.uint32), want_sc.view(np.uint32)), what


# -------------------------------------------------------------------------------------------------------- 1. inverse norms
def _norm_rows(n, f, bias, seed):
    """[n, f]: by row number modulo 8 -- ROUNDED, EXACT, zero, only the bias column, ROUNDED x 2^60, ROUNDED x 2^-60, small float32
    subnormals (the inverse norm overflows), ROUNDED."""
    rng = np.random.default_rng(seed)
    M = ref.rounded_factors(n, f, seed)
    kind = np.arange(n) % 8
    M[kind == 1] = ref.exact_factors(n, f, seed + 1)[kind == 1]
    M[kind == 2] = 0
    M[kind == 3, bias:] = 0
    M[kind == 4] *= np.float32(2.0 ** 60)
    M[kind == 5] *= np.float32(2.0 ** -60)
    sub = (rng.integers(1, 1000, (n, f)) * 2.0 ** -149).astype(np.float32)
    assert (sub > 0).all() and (sub < 2.0 ** -135).all()
    M[kind == 6] = sub[kind == 6]
    return M, kind


@case
def test_row_inv_norms(f, bias, extra):
    _lib, lib, _ptr, _stream = _api()
    ld = _ld(f, extra)
    cap, per = (_constant(name, "recmodel_amd/csrc/wmf_similar.hip") for name in ("WMF_NORMS_GRID", "WMF_NORMS_ROWS"))
    n_max = cap * per + 1
    M, kind = _norm_rows(n_max, f, bias, 100 * f + bias)
    P = ref.padded(M, ld)
    P[:, f:] = 7.0                                                   # padding is no feature, whatever it holds
    Md = _dev(P)
    want = sref.inv_norms_ref(M, bias)
    assert (want[kind == 2] == 0).all() and (want[kind == 6] == 0).all() and (not bias or (want[kind == 3] == 0).all())
    if f > bias:
        assert (want[(kind == 0) | (kind == 4) | (kind == 5) | (kind == 7)] > 0).all() and np.isfinite(want).all()
    worst = 0
    for n in (1, 63, 64, 65, n_max):
        out = torch.full((n + 1,), SENTINEL, dtype=torch.float32, device="cuda")
        _lib.check(lib.wmf_row_inv_norms(_ptr(Md), n, f, ld, bias, _ptr(out), _stream()))
        got = out.cpu().numpy()
        assert got[n] == SENTINEL
        got = got[:n]
        zero = want[:n] == 0
        assert (got[zero].view(np.uint32) == 0).all(), (f, bias, ld, n, np.flatnonzero(got[zero] != 0)[:5])
        ulps = np.abs(got[~zero].view(np.int32).astype(np.int64) - want[:n][~zero].view(np.int32).astype(np.int64))
        assert (got[~zero] > 0).all() and (ulps.size == 0 or ulps.max() <= 1), (f, bias, ld, n, int(ulps.max()))
        worst = max(worst, int(ulps.max()) if ulps.size else 0)
        if n == n_max:                                               # two runs, the same bits
            again = torch.full((n + 1,), SENTINEL, dtype=torch.float32, device="cuda")
            _lib.check(lib.wmf_row_inv_norms(_ptr(Md), n, f, ld, bias, _ptr(again), _stream()))
            assert np.array_equal(again.cpu().numpy()[:n].view(np.uint32), got.view(np.uint32))
    record_error("similar_row_inv_norms_ulps", **{f"f{f}_bias{bias}_ld{ld}": worst})


# ----------------------------------------------------------------------------------------------------- 2. the EXACT class
@case
def test_similar_topn_exact(f, bias, extra):
    """Queries that are rows of the catalogue; topn = 10; no scales, the reference inverse norms, and powers of two that make
    different integer dots tie: rows, scores and counts bit for bit, at both slice counts, with and without the row itself."""
    ld = _ld(f, extra)
    C, D = _catalogue(f, "exact"), _exact_dots(f, bias)
    excluded_self = ties = 0
    for name, scales in _scale_settings(C, bias).items():
        S = _scaled(D, scales, QUERIES)
        if name == "powers":                                         # equal scores of different integer dots
            for b in range(N_QUERIES):
                order = np.argsort(S[b], kind="stable")
                ties += int(((np.diff(S[b][order]) == 0) & (np.diff(D[b][order]) != 0)).sum())
        sim = _Similar(C, C, f, ld, bias, QUERIES, scales)
        for exclude_self in (0, 1):
            first = None
            for n_slices in (0, 3):
                got = sim(N_QUERIES, N_ROWS, 10, n_slices, exclude_self)
                if first is None:
                    first = got
                    _check_exact(got, S, QUERIES, exclude_self, None, N_ROWS, 10, (f, bias, ld, name, exclude_self, n_slices))
                    assert (got[2] == 10).all()
                    if exclude_self:
                        assert not (got[0] == QUERIES[:, None]).any()
                    else:
                        excluded_self += int((got[0] == QUERIES[:, None]).sum())
                else:
                    assert _same_bits(got, first), (f, bias, ld, name, exclude_self, n_slices)
    assert excluded_self > 0                                         # without the flag, rows do find themselves
    assert ties > 0 or f - bias < 4


# ------------------------------------------------------------------------------------------------------------ 3. the grid
@pytest.mark.parametrize("f,bias", GRID_CASES)
def test_similar_topn_grid(f, bias):
    """Query counts around the 16 rows of a wave, catalogue lengths around the tile and the stage (a one-row catalogue: its only
    row is the first query itself), every topn class, every slice count; cosine scales, the row itself left out."""
    ld = _ld(f)
    C, D = _catalogue(f, "exact"), _exact_dots(f, bias)
    scales = _scale_settings(C, bias)["norms"]
    S = _scaled(D, scales, QUERIES)
    sim = _Similar(C, C, f, ld, bias, QUERIES, scales)
    short = 0
    for nq in GRID_QUERIES:
        for ni in GRID_ROWS:
            for topn in GRID_TOPN:
                first = None
                for n_slices in GRID_SLICES:
                    got = sim(nq, ni, topn, n_slices, 1)
                    if first is None:
                        first = got
                        _check_exact(got, S, QUERIES[:nq], 1, None, ni, topn, (f, bias, nq, ni, topn, n_slices))
                        short += int((got[2] < topn).sum())
                        if ni == 1:
                            assert got[2][0] == 0 and (got[0][0] == -1).all() and (got[1][0] == -np.inf).all()
                            assert (got[2][1:] == 1).all()
                    else:
                        assert _same_bits(got, first), (f, bias, nq, ni, topn, n_slices)
    assert short


# ------------------------------------------------------------------------------------------------------ 4. exclusion lists
@pytest.mark.parametrize("f,bias", GRID_CASES + ((5, 1),))
def test_similar_topn_exclusion_lists(f, bias):
    ld = _ld(f)
    C, D = _catalogue(f, "exact"), _exact_dots(f, bias)
    scales = _scale_settings(C, bias)["norms"]
    S = _scaled(D, scales, QUERIES)
    sim = _Similar(C, C, f, ld, bias, QUERIES, scales)
    rng = np.random.default_rng(4000 + 2 * f + bias)
    for shift in range(0, N_PATTERNS, 3):
        base = _seen_rows(rng, S, N_ROWS, shift)                     # (exclusion rows: the seen-row patterns of the recommend tests)
        without = [row[row != q] for row, q in zip(base, QUERIES)]
        with_self = [np.sort(np.append(row, q)) for row, q in zip(without, QUERIES)]
        for excl in (without, with_self):
            for exclude_self in (0, 1):
                for topn, n_slices in ((10, 0), (128, 3)):
                    got = sim(N_QUERIES, N_ROWS, topn, n_slices, exclude_self, excl)
                    _check_exact(got, S, QUERIES, exclude_self, excl, N_ROWS, topn, (f, bias, shift, excl is with_self, exclude_self, topn))
    # the same answer whether the row itself is excluded by the flag, by its list, or by both
    a = sim(N_QUERIES, N_ROWS, 10, 0, 1, without)
    assert _same_bits(a, sim(N_QUERIES, N_ROWS, 10, 0, 0, with_self)) and _same_bits(a, sim(N_QUERIES, N_ROWS, 10, 0, 1, with_self))


# ----------------------------------------------------------------------------------------- 5. the tie to wmf_recommend_topn
def _recommend(Ud, Id, f, ld, user_idx, n_users, n_items, topn, n_slices):
    _lib, lib, _ptr, _stream = _api()
    ws = torch.empty(int(lib.wmf_recommend_workspace_bytes(n_users, topn, n_slices)), dtype=torch.uint8, device="cuda")
    items = torch.full((n_users, topn), -7, dtype=torch.int32, device="cuda")
    sc = torch.full((n_users, topn), SENTINEL, dtype=torch.float32, device="cuda")
    cnt = torch.full((n_users,), -7, dtype=torch.int32, device="cuda")
    _lib.check(lib.wmf_recommend_topn(_ptr(Ud), _ptr(Id), f, ld, 0, _ptr(user_idx), n_users, n_items, None, None, topn, n_slices, _ptr(items),
                                      _ptr(sc), _ptr(cnt), _ptr(ws), ws.numel(), _stream()))
    return items.cpu().numpy(), sc.cpu().numpy(), cnt.cpu().numpy()


@case
def test_similar_topn_is_the_recommend_scan(f, bias, extra):
    """ROUNDED class, no scales, the row itself allowed.  bias = 0: the bits of wmf_recommend_topn(bias = 0) on the same buffers.
    bias = 1: the bits of wmf_recommend_topn(bias = 0) on copies whose column 0 is zero -- a zero column adds exact zeros to the
    same MFMA chain."""
    ld = _ld(f, extra)
    C = _catalogue(f, "rounded")
    sim = _Similar(C, C, f, ld, bias, QUERIES)
    Zd = sim.Cd
    if bias:
        Zd = sim.Cd.clone()
        Zd[:, 0] = 0
    for topn, n_slices in ((10, 0), (128, 3)):
        got = sim(N_QUERIES, N_ROWS, topn, n_slices, 0)
        want = _recommend(Zd, Zd, f, ld, sim.query_idx, N_QUERIES, N_ROWS, topn, n_slices)
        assert _same_bits(got, want), (f, bias, ld, topn, n_slices)


# ----------------------------------------------------------------------------------------------- 6. the ROUNDED class, cosine
@case
def test_similar_topn_rounded_cosine(f, bias, extra):
    """Inverse norms from wmf_row_inv_norms on the device.  Positions unique, best first by the device's own scores, every score
    within B_cos of the float64 cosine, the order within B_cos; without self-exclusion the row finds itself with a score within
    B_cos of 1 (unless another row's cosine is within the bound of 1 as well: at one feature every cosine is 1 or -1)."""
    _lib, lib, _ptr, _stream = _api()
    ld = _ld(f, extra)
    C = _catalogue(f, "rounded")
    cos, B = _rounded_cosines(f, bias)
    sim = _Similar(C, C, f, ld, bias, QUERIES)
    inv = torch.empty(N_ROWS, dtype=torch.float32, device="cuda")
    _lib.check(lib.wmf_row_inv_norms(_ptr(sim.Cd), N_ROWS, f, ld, bias, _ptr(inv), _stream()))
    sim.scales = (inv, inv)
    worst_score = worst_order = 0.0
    found = 0
    for exclude_self in (0, 1):
        first = None
        for topn, n_slices in ((10, 0), (10, 3)):
            what = (f, bias, ld, exclude_self, topn, n_slices)
            rows, sc, cnt = got = sim(N_QUERIES, N_ROWS, topn, n_slices, exclude_self)
            if first is not None:
                assert _same_bits(got, first), what                  # (and two runs of the same call, below)
                continue
            first = got
            assert _same_bits(sim(N_QUERIES, N_ROWS, topn, n_slices, exclude_self), got), what
            assert (cnt == topn).all()
            for b, q in enumerate(QUERIES):
                elig = np.setdiff1d(np.arange(N_ROWS), [q]) if exclude_self else np.arange(N_ROWS)
                it = rows[b].astype(np.int64)
                assert np.isin(it, elig).all() and len(np.unique(it)) == topn, (what, b)
                worst_score = max(worst_score, float((np.abs(sc[b].astype(np.float64) - cos[b, it]) / B[b, it]).max()))
                assert (np.diff(sc[b]) <= 0).all(), (what, b)
                worst_order = max(worst_order, _check_rounded_order(np.searchsorted(elig, it), cos[b, elig], B[b, elig], (what, b)))
                if not exclude_self:
                    others = np.delete(np.arange(N_ROWS), q)
                    if (1.0 - cos[b, others] > 2 * B[b, others] + 2 * B[b, q]).all():
                        assert q in it and abs(float(sc[b][it == q][0]) - 1.0) <= B[b, q], (what, b)
                        found += 1
    assert worst_score <= 1.0, (f, bias, ld, worst_score)
    assert found == N_QUERIES or f - bias == 1
    record_error("similar_scan_kernel", **{f"f{f}_bias{bias}_ld{ld}": worst_score})
    record_error("similar_order", **{f"f{f}_bias{bias}_ld{ld}": worst_order})


# ------------------------------------------------------------------------------------------------------- 7. two matrices
@pytest.mark.parametrize("f,bias", GRID_CASES + ((5, 1),))
def test_similar_topn_two_matrices(f, bias):
    """Queries from another matrix of the same width, in an order that is not the row order: q_inv_norm is indexed by the row id.
    exclude_self then leaves out the catalogue row with the query's id."""
    ld = _ld(f)
    C = _catalogue(f, "exact")
    Q = ref.exact_factors(50, f, 10 * f + 3)
    query_rows = np.random.default_rng(f).permutation(50)[:N_QUERIES]
    query_rows[7] = query_rows[3]
    D = sref.dot_matrix_int(Q, C, query_rows, np.arange(N_ROWS), bias)
    sq = (2.0 ** (np.arange(50) % 5)).astype(np.float32)
    si = (2.0 ** -(np.arange(N_ROWS) % 3)).astype(np.float32)
    assert len(np.unique(sq[query_rows[:5]])) > 1 and not np.array_equal(sq[query_rows], sq[:N_QUERIES])
    S = sref.scale_f32(D, sq[query_rows], si)
    sim = _Similar(Q, C, f, ld, bias, query_rows, (sq, si))
    for exclude_self in (0, 1):
        for topn, n_slices in ((10, 0), (64, 2)):
            got = sim(N_QUERIES, N_ROWS, topn, n_slices, exclude_self)
            _check_exact(got, S, query_rows, exclude_self, None, N_ROWS, topn, (f, bias, exclude_self, topn))


# ------------------------------------------------------------------------------------------------- 8. optional outputs
def test_similar_topn_without_scores_and_counts():
    f, bias = 129, 1
    C, D = _catalogue(f, "exact"), _exact_dots(f, bias)
    scales = _scale_settings(C, bias)["norms"]
    S = _scaled(D, scales, QUERIES)
    sim = _Similar(C, C, f, _ld(f), bias, QUERIES, scales)
    full = sim(N_QUERIES, N_ROWS, 10, 0, 1)
    for scores, count in ((False, True), (True, False), (False, False)):
        got = sim(N_QUERIES, N_ROWS, 10, 2, 1, None, scores=scores, count=count)
        _check_exact(got, S, QUERIES, 1, None, N_ROWS, 10, (scores, count))
        assert np.array_equal(got[0], full[0])


# ----------------------------------------------------------------------------------------------------- 9. refused calls
def test_similar_entry_points_refuse_bad_arguments():
    """Every WMF_EINVAL case of the header, with a null stream: nothing can have been enqueued.  The pointers are real."""
    _lib, lib, _ptr, _ = _api()
    f, ld, n, nq, topn = 16, 16, 64, 8, 10
    M = torch.zeros(n, ld, dtype=torch.float32, device="cuda")
    inv = torch.zeros(n, dtype=torch.float32, device="cuda")
    qi = torch.zeros(nq, dtype=torch.int32, device="cuda")
    ip = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
    ix = torch.zeros(1, dtype=torch.int32, device="cuda")
    rows = torch.full((nq, topn), -7, dtype=torch.int32, device="cuda")
    ws_bytes = int(lib.wmf_similar_workspace_bytes(nq, topn, 0))
    assert ws_bytes == int(lib.wmf_recommend_workspace_bytes(nq, topn, 0)) > 0
    assert int(lib.wmf_similar_workspace_bytes(nq, topn, 3)) == int(lib.wmf_recommend_workspace_bytes(nq, topn, 3))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    good = dict(queries=_ptr(M), catalogue=_ptr(M), f=f, ld=ld, bias=0, sq=None, si=None, qi=_ptr(qi), nq=nq, n=n, self_=1, ip=None, ix=None,
                topn=topn, slices=0, rows=_ptr(rows), sc=None, cnt=None, ws=_ptr(ws), ws_bytes=ws_bytes)

    def call(**change):
        a = dict(good, **change)
        return lib.wmf_similar_topn(a["queries"], a["catalogue"], a["f"], a["ld"], a["bias"], a["sq"], a["si"], a["qi"], a["nq"], a["n"], a["self_"],
                                    a["ip"], a["ix"], a["topn"], a["slices"], a["rows"], a["sc"], a["cnt"], a["ws"], a["ws_bytes"], None)
    bad = [dict(ld=18), dict(f=20), dict(f=0), dict(ld=276, f=261), dict(queries=None), dict(catalogue=None), dict(qi=None), dict(rows=None),
           dict(ws=None), dict(sq=_ptr(inv)), dict(si=_ptr(inv)), dict(ip=_ptr(ip)), dict(ix=_ptr(ix)), dict(nq=0), dict(n=0), dict(n=2 ** 31),
           dict(topn=0), dict(topn=129), dict(slices=-1), dict(slices=257), dict(ws_bytes=ws_bytes - 1), dict(slices=65, ws_bytes=ws_bytes)]
    for change in bad:
        assert call(**change) == _lib.WMF_EINVAL, change
        with pytest.raises(ValueError):
            _lib.check(call(**change))
    for change in (dict(ld=18), dict(f=20), dict(n=-1), dict(M=None), dict(out=None)):
        a = dict(dict(M=_ptr(M), n=n, f=f, ld=ld, out=_ptr(inv)), **change)
        assert lib.wmf_row_inv_norms(a["M"], a["n"], a["f"], a["ld"], 0, a["out"], None) == _lib.WMF_EINVAL, change
    torch.cuda.synchronize()
    assert (rows.cpu().numpy() == -7).all() and (inv.cpu().numpy() == 0).all()
    assert lib.wmf_row_inv_norms(None, 0, f, ld, 0, None, None) == 0                      # no rows: a no-op
