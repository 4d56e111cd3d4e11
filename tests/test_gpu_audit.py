"""wmf_half_step_audit / wmf_half_step_audit_f64 through the C ABI (csrc/wmf_audit.hip), per number, against tests/audit_ref.py.

The vocabulary of tests/test_gpu_serving.py: WIDTHS has every trip count of a 16-lane walk over a row's 16-byte pieces (1 .. 5
pieces per lane: the kernel's five instantiations), LD_EXTRA the wider leading dimensions, both bias settings.  Two input classes:
EXACT -- integer factors, integer weights and an integer dense term, ranges for which audit_ref asserts that every sum of
magnitudes stays below 2^53, so every partial sum in any order is exact and the device must give audit_ref's bits -- and
GAUSSIAN -- standard-normal factors, the sums within 1e-10 relative and eta within 1e-12 absolute of audit_ref: float64 summation
over at most 1e5 terms of one sign moves a sum by at most 1e5 * 2^-53 = 1.1e-11 relative, a tenfold margin gives 1e-10; eta is
a ratio of square roots of such sums and at most 1, so a relative 1e-11 of it stays below 1e-12 * 10.

Row lengths 0, 1, 3, 4, 5 (the four entries in flight), 63, 64, 65, and 4095, 4096, 4097, 9000 around the hand-over to the
workgroup kernel; row counts 1, 3, 4, 5 (the four waves of a workgroup) and once past the grid cap of 2048 workgroups.  Every
output sits between sentinels."""
import functools

import numpy as np
import pytest
import torch

import audit_ref
import serving_ref as sref
from test_gpu_serving import LD_EXTRA, WIDTHS

pytestmark = pytest.mark.gpu

CASES = [(f, b, 0) for f in WIDTHS for b in (0, 1)] + [(f, b, e) for f, e in LD_EXTRA.items() for b in (0, 1)]
case = pytest.mark.parametrize("f,bias,extra", CASES, ids=[f"f{f}-b{b}" + (f"-ld+{e}" if e else "") for f, b, e in CASES])
F64_WIDTHS = (1, 5, 64, 129, 260)
N_ITEMS = 300
SHORT = (0, 1, 3, 4, 5, 63, 64, 65, 0)                             # empty first and last rows
LONG = (0, 4095, 4096, 4097, 2, 9000, 0)
SENTINEL = -12345.0
LAMBDA = 0.1


# ------------------------------------------------------------------------------------------------------------------ helpers
def _api():
    from recmodel_amd import _lib
    from recmodel_amd.engine import _ptr, _stream
    return _lib, _lib.load(), _ptr, _stream


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _csr(lengths, seed, n_items=N_ITEMS, max_weight=5):
    """Rows of the given lengths: columns drawn with replacement (duplicates occur), integer weights 0 .. max_weight (stored zeros
    occur).  One spare element keeps the arrays of an all-empty matrix valid."""
    rng = np.random.default_rng(seed)
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    nnz = int(indptr[-1])
    indices = rng.integers(0, n_items, nnz + 1).astype(np.int32)
    values = rng.integers(0, max_weight + 1, nnz + 1).astype(np.float64)
    return indptr, indices, values


def _small_ints(n, f, seed):
    """Integers in -1 .. 1: the range that keeps a 9000-entry row exact at every width."""
    return np.random.default_rng(seed).integers(-1, 2, (n, f)).astype(np.float32)


def _run(X, Y, f, ld, bias, indptr, indices, values, dense, rows, f64=False, lo=0, n=None):
    """One call on rows [lo, lo + n) of the CSR through a window of indptr.  X, Y, dense are host arrays [., f]; ld: the leading
    dimension of the float32 factors.  Returns (sums [3], rows [n, 3] or None); checks the sentinels around both."""
    _lib, lib, _ptr, _stream = _api()
    n_all = len(indptr) - 1
    n = n_all - lo if n is None else n
    if f64:
        Xd, Yd, vd = _dev(X, np.float64), _dev(Y, np.float64), _dev(values, np.float64)
    else:
        Xd, Yd, vd = _dev(sref.padded(X, ld)), _dev(sref.padded(Y, ld)), _dev(values, np.float32)
    ipd, ixd = _dev(indptr, np.int64), _dev(indices, np.int32)
    out_sums = torch.full((5,), SENTINEL, dtype=torch.float64, device="cuda")
    out_rows = torch.full((3 * n + 2,), SENTINEL, dtype=torch.float64, device="cuda") if rows else None
    dd = _dev(dense, np.float64) if rows else None
    ws_bytes = int(lib.wmf_audit_workspace_bytes(n))
    ws = torch.empty(ws_bytes + 64, dtype=torch.uint8, device="cuda")
    ws[ws_bytes:] = 0x5A
    win = ipd[lo: lo + n + 1]
    if f64:
        rc = lib.wmf_half_step_audit_f64(_ptr(Xd[lo:]) if n_all > lo else _ptr(Xd), _ptr(Yd), f, bias, _ptr(win), _ptr(ixd), _ptr(vd), n,
                                         _ptr(dd[lo:]) if rows and n_all > lo else _ptr(dd), _ptr(out_sums[1:]),
                                         _ptr(out_rows[1:]) if rows else None, _ptr(ws), ws_bytes, _stream())
    else:
        rc = lib.wmf_half_step_audit(_ptr(Xd[lo:]) if n_all > lo else _ptr(Xd), _ptr(Yd), f, ld, bias, _ptr(win), _ptr(ixd), _ptr(vd), n,
                                     _ptr(dd[lo:]) if rows and n_all > lo else _ptr(dd), _ptr(out_sums[1:]),
                                     _ptr(out_rows[1:]) if rows else None, _ptr(ws), ws_bytes, _stream())
    _lib.check(rc)
    sums = out_sums.cpu().numpy()
    assert sums[0] == SENTINEL and sums[4] == SENTINEL
    assert bool((ws[ws_bytes:] == 0x5A).all())
    got_rows = None
    if rows:
        r = out_rows.cpu().numpy()
        assert r[0] == SENTINEL and r[-1] == SENTINEL
        got_rows = r[1:-1].reshape(n, 3)
    return sums[1:4], got_rows


def _ld(f, extra=0):
    return (f + 3) // 4 * 4 + extra


def _window(indptr, lo, n):
    return np.asarray(indptr[lo: lo + n + 1])


def _check_exact(X, Y, f, ld, bias, indptr, indices, values, dense, f64=False, lo=0, n=None):
    """Both output modes on rows [lo, lo + n), bit for bit against audit_ref."""
    n = len(indptr) - 1 - lo if n is None else n
    want_sums, want_rows = audit_ref.half_step_audit(X[lo: lo + n], Y, bias, _window(indptr, lo, n), indices, values, dense[lo: lo + n])
    for rows in (False, True):
        sums, got_rows = _run(X, Y, f, ld, bias, indptr, indices, values, dense, rows, f64, lo, n)
        assert np.array_equal(sums, want_sums), (rows, sums, want_sums)
        if rows:
            assert np.array_equal(got_rows, want_rows), np.flatnonzero((got_rows != want_rows).any(axis=1))[:10]


@functools.lru_cache(maxsize=None)
def _exact_inputs(f, n, lengths_key, seed, small):
    lengths = {"short": SHORT, "long": LONG}.get(lengths_key, lengths_key)
    make = _small_ints if small else sref.exact_factors
    X, Y = make(n, f, seed + 1), make(N_ITEMS, f, seed + 2)
    indptr, indices, values = _csr(lengths, seed + 3, max_weight=2 if small else 5)
    dense = np.random.default_rng(seed + 4).integers(-50, 51, (n, f)).astype(np.float64)
    for a in (X, Y, indptr, indices, values, dense):
        a.setflags(write=False)
    return X, Y, indptr, indices, values, dense


# -------------------------------------------------------------------------------------------------------------------- EXACT
@case
def test_integer_inputs_bit_for_bit(f, bias, extra):
    X, Y, indptr, indices, values, dense = _exact_inputs(f, len(SHORT), "short", 100 * f, False)
    _check_exact(X, Y, f, _ld(f, extra), bias, indptr, indices, values, dense)


@pytest.mark.parametrize("f,bias", [(5, 0), (5, 1), (129, 1), (260, 0)])
def test_rows_around_the_workgroup_threshold(f, bias):
    """4095 and 4096 entries stay with their wave, 4097 and 9000 go to the list and a workgroup each (at one and at five pieces
    per lane); the rows between and after them are unaffected."""
    X, Y, indptr, indices, values, dense = _exact_inputs(f, len(LONG), "long", 7 * f + bias, True)
    _check_exact(X, Y, f, _ld(f), bias, indptr, indices, values, dense)
    if f in F64_WIDTHS:
        _check_exact(X, Y, f, None, bias, indptr, indices, values, dense, f64=True)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 4 * 2048 + 5])
def test_row_counts(n):
    """The four waves of a workgroup, and rows that a wave reaches only in a later trip of the grid-stride loop."""
    lengths = tuple([0] + [(3 * r) % 7 for r in range(1, n - 1)] + ([0] if n > 1 else []))
    X, Y, indptr, indices, values, dense = _exact_inputs(5, n, lengths, 11 + n, False)
    _check_exact(X, Y, 5, 8, 1, indptr, indices, values, dense)


def test_all_rows_empty():
    X, Y, indptr, indices, values, dense = _exact_inputs(5, 6, (0,) * 6, 3, False)
    for f64 in (False, True):
        sums, rows = _run(X, Y, 5, 8, 0, indptr, indices, values, dense, True, f64)
        assert np.array_equal(sums, np.zeros(3))
        assert np.array_equal(rows[:, 0], (dense ** 2).sum(axis=1)) and not rows[:, 1:].any()


@pytest.mark.parametrize("lo,n", [(0, 9), (2, 5), (8, 1), (0, 1), (3, 0), (1, 8)])
def test_indptr_windows(lo, n):
    """Rows [lo, lo + n) of a longer CSR: the window's pointers index the whole index and value arrays."""
    X, Y, indptr, indices, values, dense = _exact_inputs(65, len(SHORT), "short", 41, False)
    _check_exact(X, Y, 65, 68, 1, indptr, indices, values, dense, lo=lo, n=n)
    _check_exact(X, Y, 65, None, 1, indptr, indices, values, dense, f64=True, lo=lo, n=n)


@pytest.mark.parametrize("f", F64_WIDTHS)
@pytest.mark.parametrize("bias", [0, 1])
def test_float64_entry_point_bit_for_bit(f, bias):
    X, Y, indptr, indices, values, dense = _exact_inputs(f, len(SHORT), "short", 100 * f, False)
    _check_exact(X, Y, f, None, bias, indptr, indices, values, dense, f64=True)


# ----------------------------------------------------------------------------------------------------------------- GAUSSIAN
def _gaussian_inputs(f, lengths, seed):
    n = len(lengths)
    X, Y = sref.rounded_factors(n, f, seed + 1), sref.rounded_factors(N_ITEMS, f, seed + 2)
    indptr, indices, _ = _csr(lengths, seed + 3)
    values = np.random.default_rng(seed + 4).uniform(0.0, 40.0, len(indices)).astype(np.float32)
    return X, Y, indptr, indices, values


def _check_gaussian(X, Y, f, ld, bias, indptr, indices, values, f64=False):
    A = audit_ref.gram(Y, bias) + LAMBDA * np.eye(f)
    dense = X.astype(np.float64) @ A
    want_sums, want_rows = audit_ref.half_step_audit(X, Y, bias, indptr, indices, values, dense)
    want_eta = audit_ref.eta_from_rows(want_rows, X, np.linalg.norm(A))
    sums0, _ = _run(X, Y, f, ld, bias, indptr, indices, values, dense, False, f64)
    sums, rows = _run(X, Y, f, ld, bias, indptr, indices, values, dense, True, f64)
    assert np.array_equal(sums, sums0)                             # the sums do not depend on the output mode
    assert sums[2] == want_sums[2]
    assert np.all(np.abs(sums[:2] - want_sums[:2]) <= 1e-10 * np.abs(want_sums[:2])), (sums, want_sums)
    eta = audit_ref.eta_from_rows(rows, X, np.linalg.norm(A))
    assert np.max(np.abs(eta - want_eta)) <= 1e-12, np.max(np.abs(eta - want_eta))
    return sums, rows


@case
def test_gaussian_factors(f, bias, extra):
    X, Y, indptr, indices, values = _gaussian_inputs(f, SHORT, 10 * f + bias)
    _check_gaussian(X, Y, f, _ld(f, extra), bias, indptr, indices, values)


@pytest.mark.parametrize("f,bias", [(5, 1), (64, 0), (129, 1), (260, 0)])
def test_gaussian_factors_float64_and_long_rows(f, bias):
    X, Y, indptr, indices, values = _gaussian_inputs(f, LONG + SHORT, 10 * f + bias)
    _check_gaussian(X, Y, f, None, bias, indptr, indices, values, f64=True)
    _check_gaussian(X, Y, f, _ld(f), bias, indptr, indices, values)


@pytest.mark.parametrize("f64", [False, True])
def test_two_runs_are_bit_identical(f64):
    """Eight listed rows: the order in which their workgroups finish and the order of the list may differ from run to run, the
    results may not."""
    lengths = (5000, 3, 4100, 0, 4097, 70, 6000, 4500, 9, 4200, 4300, 8000, 1)
    X, Y, indptr, indices, values = _gaussian_inputs(129, lengths, 77)
    first = _check_gaussian(X, Y, 129, 132, 1, indptr, indices, values, f64)
    for _ in range(2):
        again = _check_gaussian(X, Y, 129, 132, 1, indptr, indices, values, f64)
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
