"""tests/f64_ref.py -- the reference the float64 GPU tests are gated on -- against three independent statements of the same row:
mpmath at 40 digits, the project's NumPy oracle (oracle/wmf_oracle.py, float64), and the reference implementation's own
float64 rows (golden half_par.npz, whose first Gramian is a float32 product: 2e-5)."""
import fractions

import numpy as np
import pytest
import scipy.sparse as sp

import f64_ref
from conftest import csr_from, load_golden
from oracle import wmf_oracle as orc

LAMBDA = 0.1


def _ragged(n, m, seed, lengths=None):
    """Rows of 0 .. 2 m entries: a stored zero in row 1, a duplicated column in row 2, columns with replacement beyond m."""
    rng = np.random.default_rng(seed)
    deg = np.asarray(lengths if lengths is not None else rng.integers(0, 2 * m, n))
    deg[0] = 0
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    indices = np.concatenate([rng.choice(m, d, replace=d > m) for d in deg] + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    values = 10 * np.log(1 + rng.integers(1, 8, indptr[-1])).astype(np.float64)
    if deg[1] > 0:
        values[indptr[1]] = 0.0
    if deg[2] > 1:
        indices[indptr[2] + 1] = indices[indptr[2]]
    return indptr, indices, values


def _mp_row(Y, bias, lam, idx, vals):
    """x_u, tau_u and the backward error of a given x at 40 digits."""
    import mpmath as mp
    mp.mp.dps = 40
    f = Y.shape[1]
    Yt = [[mp.mpf(1) if (bias and c == 0) else mp.mpf(float(Y[r, c])) for c in range(f)] for r in range(Y.shape[0])]
    G = mp.matrix(f, f)
    for row in Yt:
        for i in range(f):
            for j in range(f):
                G[i, j] += row[i] * row[j]
    for i in range(f):
        G[i, i] += mp.mpf(lam)
    A, b = G.copy(), mp.matrix(f, 1)
    ws = []
    for e, c in zip(idx, vals):
        w = mp.mpf(float(np.float64(c) - Y[e, 0])) if bias else mp.mpf(float(c))   # (the float64 difference, as stored arithmetic)
        ws.append(w)
        for i in range(f):
            b[i] += (w + 1) * Yt[e][i]
            for j in range(f):
                A[i, j] += w * Yt[e][i] * Yt[e][j]
    x = mp.lu_solve(A, b)
    Ginv = G ** -1
    tau = mp.mpf(0)
    for e, w in zip(idx, ws):
        y = mp.matrix(Yt[e])
        tau += abs(w) * (y.T * Ginv * y)[0]

    def eta(xg):
        xv = mp.matrix([mp.mpf(float(v)) for v in xg])
        r = A * xv - b
        return float(mp.norm(r) / (mp.mnorm(A, "f") * mp.norm(xv) + mp.norm(b)))
    return np.array([float(v) for v in x]), float(tau), eta


@pytest.mark.parametrize("f,bias", [(1, 0), (2, 1), (5, 0), (7, 1), (16, 0), (16, 1)])
def test_rows_against_mpmath_at_forty_digits(f, bias):
    m = 2 * f + 7
    rng = np.random.default_rng(40 + f)
    Y = rng.random((m, f))
    if bias:
        Y[:, 0] = np.linspace(-5, 30, m)                             # weights below zero too
    indptr, indices, values = _ragged(6, m, 7 + f, lengths=[0, 1, 4, 33, 2 * m + 3, 9])
    probe = rng.random((6, f))                                       # any x: its backward error is a number of its own
    ref = f64_ref.half_step(Y, bias, LAMBDA, indptr, indices, values, candidates=(probe,), want_cond=True)
    assert not ref["x"][0].any() and ref["tau"][0] == 0
    for u in range(1, 6):
        lo, hi = indptr[u], indptr[u + 1]
        x, tau, eta = _mp_row(Y, bias, LAMBDA, indices[lo:hi], values[lo:hi])
        # the reference rounds x to float64 (2^-53 per element) after refinement; cond * 2^-64 is what the longdouble residual leaves
        bound = 4 * np.finfo(np.float64).eps + ref["cond"][u] * 2.0 ** -60
        assert np.linalg.norm(ref["x"][u] - x) <= bound * np.linalg.norm(x), (u, np.linalg.norm(ref["x"][u] - x) / np.linalg.norm(x))
        assert abs(ref["tau"][u] - tau) <= 1e-9 * tau
        assert abs(ref["eta"][0, u] - eta(probe[u])) <= 1e-9 * eta(probe[u])
        # eta of an almost exact x is of the order of float64 rounding; longdouble resolves it to a few per cent
        e_np = eta(ref["x_numpy"][u])
        assert abs(ref["eta_numpy"][u] - e_np) <= 0.05 * e_np + 1e-19, (ref["eta_numpy"][u], e_np)
        assert e_np <= 1e-15


@pytest.mark.parametrize("bias", [0, 1])
@pytest.mark.parametrize("f", [3, 37, 130])
def test_rows_against_the_numpy_oracle(f, bias):
    m, n = 2 * f + 7, 14
    rng = np.random.default_rng(f)
    Y = rng.random((m, f))
    indptr, indices, values = _ragged(n, m, 100 + f)
    C = sp.csr_matrix((values, indices, indptr), shape=(n, m))
    # (the constructor keeps the arrays as stored: the oracle reads indptr / indices / data)
    want = (orc.recompute_factors_bias if bias else orc.recompute_factors)(Y, C, LAMBDA, dtype="float64")
    ref = f64_ref.half_step(Y, bias, LAMBDA, indptr, indices, values, want_cond=True)
    err = f64_ref.row_errors(want, ref["x"])
    # the oracle is one float64 LU solve of sums taken in float64: cond * 2^-53 with a constant of the order of sqrt(entries);
    # cond <= 1e5 on these inputs (asserted), so 1e-11 * 1e5 * 2^-53 * 1e4 ...: 1e-11 has a hundredfold margin
    assert np.nanmax(ref["cond"]) <= 1e5
    assert np.all(err <= 1e-11), err.max()
    assert err[0] == 0
    # the batched float64 form is the same arithmetic as the oracle's
    short = _ragged(40, m, 300 + f, lengths=np.random.default_rng(1).integers(0, 40, 40))
    got = f64_ref.half_step_batched(Y, bias, LAMBDA, *short, batch=16)
    ref2 = f64_ref.half_step(Y, bias, LAMBDA, *short)
    assert np.all(f64_ref.row_errors(got, ref2["x"]) <= 1e-11)


def test_rows_against_the_reference_implementations_golden_rows():
    g = load_golden("half_par.npz")
    C = csr_from(g, "C")
    for bias in (0, 1):
        Y, want = g[f"items0_bias{bias}"].astype(np.float64), g[f"users_par_bias{bias}"]
        ref = f64_ref.half_step(Y, bias, LAMBDA, C.indptr, C.indices, C.data.astype(np.float64))
        np.testing.assert_allclose(ref["x"], want, rtol=2e-5, atol=2e-6)


def test_diagonal_systems_are_exact():
    """A fixed side of scaled unit vectors: every A_u is diagonal and the reference's x is b / A rounded once."""
    f, lam = 6, 0.25
    Y = np.zeros((f, f))
    for j in range(f):
        Y[j, j] = (-1.0) ** j * 2.0 ** (j - 2)
    indptr = np.array([0, 2, 3, 3])
    indices = np.array([1, 4, 5], dtype=np.int32)
    values = np.array([3.0, 0.5, 7.0])
    ref = f64_ref.half_step(Y, 0, lam, indptr, indices, values)
    F = fractions.Fraction
    for u in range(2):
        want = np.zeros(f)
        for e in range(indptr[u], indptr[u + 1]):
            j, w = indices[e], F(values[e])
            y = F(Y[j, j])
            want[j] = float((w + 1) * y / (y * y + F(lam) + w * y * y))
        assert np.array_equal(ref["x"][u], want)
    assert not ref["x"][2].any()
